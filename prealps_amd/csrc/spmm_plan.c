/*
 * spmm_plan.c -- cuts the SpMM plan of a local CSR panel (local column ids): SELL-64 slices and the
 * workgroup blocks over them, in one of three forms (pa_device.h: pa_spmm_plan_t):
 *   window  a block is a run of slices of one subdomain; its LDS window is the subdomain's own row
 *           range, or the 256 rows around the block when the subdomain is larger than that
 *           (1024-row windows measured slower);
 *   staged  every X row a block touches is copied to LDS first; 16-bit LDS slots instead of columns;
 *   runs    the staged plan with one slot per run of up to three consecutive columns.
 * Host arithmetic only (spmm_plan.h); operator.c reads the switches and uploads the result.
 * pa_spmm_plan_value_map: which panel entry every stored value is, for an update of the values in place.
 */
#include <string.h>

#include "spmm_plan.h"

static const size_t k_elem[PA_PL_COUNT] = {
  sizeof(long long), sizeof(int), sizeof(int), sizeof(int), sizeof(int), sizeof(unsigned short), sizeof(double),
  sizeof(int), sizeof(int), sizeof(int), sizeof(int), sizeof(int), sizeof(int)};

#define ARR(pl, which, type) ((type*)(pl)->a[which].p)

/* what a builder needs besides the plan's own arrays */
typedef struct {
  int* sl_part;        /* subdomain of every slice */
  char* needs_halo;    /* per block: it reads a halo row */
  int* stamp;          /* per column: the collection (gen) that last saw it */
  int* slot_of;        /* per column: its LDS slot in the block being filled */
  int gen;
  size_t ext_cap;      /* room in ext_rows */
  size_t ent_cap;      /* run plan: room for runs in col16 / val */
} scratch_t;

static void scratch_free(scratch_t* s) {
  free(s->sl_part); free(s->needs_halo); free(s->stamp); free(s->slot_of);
  memset(s, 0, sizeof(*s));
}

void pa_spmm_plan_free(pa_spmm_host_plan_t* pl) {
  for (int i = 0; i < PA_PL_COUNT; ++i) free(pl->a[i].p);
  memset(pl, 0, sizeof(*pl));
}

static void* arr_new(pa_spmm_host_plan_t* pl, int which, size_t cap) {
  pl->a[which].elem = k_elem[which];
  pl->a[which].p = pa_big_alloc(cap * k_elem[which]);
  return pl->a[which].p;
}
static void arr_set(pa_spmm_host_plan_t* pl, int which, size_t n, size_t n_alloc) {
  pl->a[which].n = n; pl->a[which].n_alloc = n_alloc;
}

/* Rows per SpMM workgroup, a multiple of 64.  The measured optimum on a full GPU is `dflt` (256; 192 for the
 * staged plan at 8 columns); a process that owns few rows (one shard of a multi-GPU run: 130 k rows are 519
 * such blocks on 256 CUs) gets smaller blocks, so that every CU has at least four workgroups to hide the
 * staging and streaming latencies.  At most cap_rows (the staging area); below 64: no such plan. */
static int block_rows(const pa_spmm_plan_in_t* in, int dflt, int cap_rows) {
  int cus = in->cus > 0 ? in->cus : 256;
  int rows = dflt;
  while (rows > 64 && (long long)in->m / rows < 4LL * cus) rows -= 64;
  if (rows < 64) rows = 64;
  rows &= ~63;
  if (rows > cap_rows) rows = cap_rows & ~63;
  return rows;
}

/* The 64-row slices, subdomain after subdomain, with the padded row length of plain SELL storage
 * (sl_len, sl_off), and room for one block per slice. */
static int cut_slices(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl, scratch_t* s) {
  int nslices = 0;
  for (int p = in->part0; p < in->part1; ++p) nslices += (in->rowPos[p + 1] - in->rowPos[p] + 63) / 64;
  size_t ns1 = (size_t)(nslices ? nslices : 1);
  long long* sl_off = (long long*)arr_new(pl, PA_PL_SL_OFF, ns1 + 1);
  int* sl_len = (int*)arr_new(pl, PA_PL_SL_LEN, ns1);
  int* sl_row0 = (int*)arr_new(pl, PA_PL_SL_ROW0, ns1);
  int* sl_nrows = (int*)arr_new(pl, PA_PL_SL_NROWS, ns1);
  int* blk_slice = (int*)arr_new(pl, PA_PL_BLK_SLICE, ns1 + 1);
  s->sl_part = (int*)malloc(ns1 * sizeof(int));
  s->needs_halo = (char*)malloc(ns1);
  if (!sl_off || !sl_len || !sl_row0 || !sl_nrows || !blk_slice || !s->sl_part || !s->needs_halo) return -1;
  int q = 0;
  sl_off[0] = 0;
  for (int p = in->part0; p < in->part1; ++p) {
    int pr0 = in->rowPos[p] - in->row_off, pr1 = in->rowPos[p + 1] - in->row_off;
    for (int r = pr0; r < pr1; r += 64, ++q) {
      int nr = pr1 - r < 64 ? pr1 - r : 64, len = 0;
      for (int i = 0; i < nr; ++i) { int l = in->rowPtr[r + i + 1] - in->rowPtr[r + i]; if (l > len) len = l; }
      sl_len[q] = len; sl_row0[q] = r; sl_nrows[q] = nr; s->sl_part[q] = p;
      sl_off[q + 1] = sl_off[q] + (long long)len * 64;
    }
  }
  pl->m = in->m; pl->nslices = nslices;
  arr_set(pl, PA_PL_SL_OFF, (size_t)nslices + 1, (size_t)nslices + 1);
  arr_set(pl, PA_PL_SL_LEN, (size_t)nslices, ns1);
  arr_set(pl, PA_PL_SL_ROW0, (size_t)nslices, ns1);
  arr_set(pl, PA_PL_SL_NROWS, (size_t)nslices, ns1);
  return 0;
}

/* Close the block list: the order in which the kernels take the blocks -- those that read no halo row
 * first, so that they can run beside the halo exchange. */
static int finish_blocks(pa_spmm_host_plan_t* pl, const scratch_t* s, int nblk) {
  size_t nb1 = (size_t)(nblk > 0 ? nblk : 1);
  int* order = (int*)arr_new(pl, PA_PL_ORDER, nb1);
  if (!order) return -1;
  int ni = 0;
  for (int b = 0; b < nblk; ++b) if (!s->needs_halo[b]) order[ni++] = b;
  int k = ni;
  for (int b = 0; b < nblk; ++b) if (s->needs_halo[b]) order[k++] = b;
  ARR(pl, PA_PL_BLK_SLICE, int)[nblk] = pl->nslices;
  pl->nblk = nblk; pl->n_interior = ni;
  arr_set(pl, PA_PL_BLK_SLICE, (size_t)nblk + 1, (size_t)nblk + 1);
  arr_set(pl, PA_PL_ORDER, (size_t)nblk, nb1);
  return 0;
}

/* ------------------------------------------------------------ window plan ---- */
static int plan_window(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl, scratch_t* s) {
  const int* rowptr = in->rowPtr;
  const int* colind = in->lcol;
  const int win_cap = 256;
  int blk_rows = block_rows(in, 256, 1 << 30);
  if (cut_slices(in, pl, s)) return -1;
  int nslices = pl->nslices;
  const long long* sl_off = ARR(pl, PA_PL_SL_OFF, long long);
  const int* sl_len = ARR(pl, PA_PL_SL_LEN, int);
  const int* sl_row0 = ARR(pl, PA_PL_SL_ROW0, int);
  const int* sl_nrows = ARR(pl, PA_PL_SL_NROWS, int);
  size_t tot = (size_t)sl_off[nslices];
  pl->sell_entries = (double)tot;
  int* scol = (int*)arr_new(pl, PA_PL_COL, tot + 64);
  double* sval = (double*)arr_new(pl, PA_PL_VAL, tot + 64);
  if (!scol || !sval) { pl->oom_entries = tot; return -1; }
  for (int q = 0; q < nslices; ++q) {
    int r = sl_row0[q], nr = sl_nrows[q], len = sl_len[q];
    int* c = scol + sl_off[q];
    double* v = sval + sl_off[q];
    for (int i = 0; i < 64; ++i) {
      int row = i < nr ? r + i : r;          /* unused lanes mirror the first row */
      int l = i < nr ? rowptr[row + 1] - rowptr[row] : 0;
      for (int k = 0; k < len; ++k) {
        if (k < l) { c[(size_t)k * 64 + i] = colind[rowptr[row] + k]; v[(size_t)k * 64 + i] = in->val[rowptr[row] + k]; }
        else { c[(size_t)k * 64 + i] = row; v[(size_t)k * 64 + i] = 0.0; } /* padding: 0 * x[row] */
      }
    }
  }
  for (size_t k = tot; k < tot + 64; ++k) { scol[k] = 0; sval[k] = 0.0; }
  arr_set(pl, PA_PL_COL, tot + 64, tot + 64);
  arr_set(pl, PA_PL_VAL, tot + 64, tot + 64);
  /* blocks */
  size_t cap_blocks = (size_t)(nslices > 0 ? nslices : 1);
  int* blk_slice = ARR(pl, PA_PL_BLK_SLICE, int);
  int* blk_win = (int*)arr_new(pl, PA_PL_BLK_WIN, 2 * cap_blocks);
  if (!blk_win) return -1;
  int nblk = 0, q = 0, max_win = 0;
  while (q < nslices) {
    int p = s->sl_part[q], q1 = q, rows = 0;
    while (q1 < nslices && s->sl_part[q1] == p && rows + 64 <= blk_rows) { rows += 64; ++q1; }
    int pr0 = in->rowPos[p] - in->row_off, pr1 = in->rowPos[p + 1] - in->row_off;
    int r0 = sl_row0[q], r1 = sl_row0[q1 - 1] + sl_nrows[q1 - 1];
    int w0, w1;
    if (pr1 - pr0 <= win_cap) { w0 = pr0; w1 = pr1; }
    else {
      int c = (r0 + r1) / 2;
      w0 = c - win_cap / 2;
      if (w0 < pr0) w0 = pr0;
      w1 = w0 + win_cap;
      if (w1 > pr1) { w1 = pr1; w0 = w1 - win_cap; }
    }
    if (w1 - w0 > max_win) max_win = w1 - w0;
    char h = 0;
    for (int k = rowptr[r0]; k < rowptr[r1] && !h; ++k) h = colind[k] >= in->m;
    blk_slice[nblk] = q; blk_win[2 * nblk] = w0; blk_win[2 * nblk + 1] = w1; s->needs_halo[nblk] = h;
    ++nblk;
    q = q1;
  }
  if (finish_blocks(pl, s, nblk)) return -1;
  arr_set(pl, PA_PL_BLK_WIN, (size_t)2 * nblk, (size_t)2 * (nblk > 0 ? nblk : 1));
  pl->win_cap = max_win;
  pl->stream_bytes = 12.0 * (double)tot;
  return 0;
}

/* ------------------------------------------------- staged and run plans ---- */
/* The rows outside [r0, r1) that rows [r0, r1) read, each once, appended to ext_rows in order of first
 * use: how many, how many of them lie below r0, and whether a halo slot is among them. */
static int collect_ext(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl, scratch_t* s, int r0, int r1,
                       int* next_out, int* nlow_out, char* halo_out) {
  pa_plan_array_t* e = &pl->a[PA_PL_EXT_ROWS];
  int* ext = (int*)e->p;
  int next = 0, nlow = 0;
  char h = 0;
  ++s->gen;
  for (int k = in->rowPtr[r0]; k < in->rowPtr[r1]; ++k) {
    int c = in->lcol[k];
    if ((c >= r0 && c < r1) || s->stamp[c] == s->gen) continue;
    s->stamp[c] = s->gen;
    if (e->n == s->ext_cap) {
      int* grown = (int*)realloc(ext, 2 * s->ext_cap * sizeof(int));
      if (!grown) return -1;
      e->p = ext = grown; s->ext_cap *= 2;
    }
    ext[e->n++] = c; ++next;
    if (c < r0) ++nlow;
    if (c >= in->m) h = 1;
  }
  *next_out = next; *nlow_out = nlow; *halo_out = h;
  return 0;
}

static void sort_ints(int* e, int n) {   /* insertion sort: the lists are short and nearly sorted */
  for (int a = 1; a < n; ++a) { int v = e[a], b = a; while (b > 0 && e[b - 1] > v) { e[b] = e[b - 1]; --b; } e[b] = v; }
}

/* staged plan: slice sq of the block over rows [r0, r1), one 16-bit LDS slot per entry */
static void fill_slots(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl, const scratch_t* s, int sq, int r0, int r1) {
  const int* rowptr = in->rowPtr;
  const long long off = ARR(pl, PA_PL_SL_OFF, long long)[sq];
  int r = ARR(pl, PA_PL_SL_ROW0, int)[sq], nr = ARR(pl, PA_PL_SL_NROWS, int)[sq], len = ARR(pl, PA_PL_SL_LEN, int)[sq];
  unsigned short* cc = ARR(pl, PA_PL_COL16, unsigned short) + off;
  double* vv = ARR(pl, PA_PL_VAL, double) + off;
  for (int i = 0; i < 64; ++i) {
    int row = i < nr ? r + i : r;
    int l = i < nr ? rowptr[row + 1] - rowptr[row] : 0;
    for (int k = 0; k < len; ++k) {
      if (k < l) {
        int c = in->lcol[rowptr[row] + k];
        cc[(size_t)k * 64 + i] = (unsigned short)((c >= r0 && c < r1) ? c - r0 : s->slot_of[c]);
        vv[(size_t)k * 64 + i] = in->val[rowptr[row] + k];
      } else { cc[(size_t)k * 64 + i] = (unsigned short)(row - r0); vv[(size_t)k * 64 + i] = 0.0; }
    }
  }
}

/* run plan: slice sq of the block over rows [r0, r1), whose staging area starts with nlow external
 * rows.  A run covers slots [s, s+2]; entries of the row that fall inside it fill its three values,
 * the rest are zeros.  Appends the slice's runs to col16 / val and sets its sl_len and sl_off. */
static int fill_runs(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl, scratch_t* s, int sq, int r0, int r1, int nlow) {
  const int* rowptr = in->rowPtr;
  const int* colind = in->lcol;
  int r = ARR(pl, PA_PL_SL_ROW0, int)[sq], nr = ARR(pl, PA_PL_SL_NROWS, int)[sq], len3 = 0;
  size_t nruns = pl->a[PA_PL_COL16].n;
  /* pass 1: runs per row */
  for (int i = 0; i < nr; ++i) {
    int row = r + i, nrun = 0, last = -4;
    for (int k = rowptr[row]; k < rowptr[row + 1]; ++k) {
      int c = colind[k], sl = (c >= r0 && c < r1) ? nlow + c - r0 : s->slot_of[c];
      if (sl > last + 2 || sl < last) { last = sl; ++nrun; }
    }
    if (nrun > len3) len3 = nrun;
  }
  if (nruns + (size_t)len3 * 64 > s->ent_cap) {
    size_t cap = (s->ent_cap + (size_t)len3 * 64) * 3 / 2;
    void* c2 = realloc(pl->a[PA_PL_COL16].p, cap * sizeof(unsigned short));
    if (!c2) return -1;
    pl->a[PA_PL_COL16].p = c2;
    void* v2 = realloc(pl->a[PA_PL_VAL].p, cap * 3 * sizeof(double));
    if (!v2) return -1;
    pl->a[PA_PL_VAL].p = v2;
    s->ent_cap = cap;
  }
  unsigned short* cc = ARR(pl, PA_PL_COL16, unsigned short) + nruns;
  double* vv = ARR(pl, PA_PL_VAL, double) + 3 * nruns;
  for (int i = 0; i < 64; ++i) {
    int row = i < nr ? r + i : r, own = nlow + row - r0, nrun = 0, last = -4;
    if (i < nr)
      for (int k = rowptr[row]; k < rowptr[row + 1]; ++k) {
        int c = colind[k], sl = (c >= r0 && c < r1) ? nlow + c - r0 : s->slot_of[c];
        if (sl > last + 2 || sl < last) {
          last = sl;
          cc[(size_t)nrun * 64 + i] = (unsigned short)sl;
          vv[((size_t)3 * nrun + 0) * 64 + i] = 0.0; vv[((size_t)3 * nrun + 1) * 64 + i] = 0.0;
          vv[((size_t)3 * nrun + 2) * 64 + i] = 0.0;
          ++nrun;
        }
        vv[((size_t)3 * (nrun - 1) + (sl - last)) * 64 + i] = in->val[k];
      }
    for (int k = nrun; k < len3; ++k) {     /* padding: zeros against the row's own slot */
      cc[(size_t)k * 64 + i] = (unsigned short)own;
      vv[((size_t)3 * k + 0) * 64 + i] = 0.0; vv[((size_t)3 * k + 1) * 64 + i] = 0.0;
      vv[((size_t)3 * k + 2) * 64 + i] = 0.0;
    }
  }
  nruns += (size_t)len3 * 64;
  ARR(pl, PA_PL_SL_LEN, int)[sq] = len3;
  ARR(pl, PA_PL_SL_OFF, long long)[sq + 1] = (long long)nruns;
  pl->a[PA_PL_COL16].n = nruns;
  return 0;
}

/* Staged plan (runs = 0) or run plan (runs = 1).  Blocks are runs of slices, which may span consecutive
 * subdomains (fewer external rows per row); a block is halved until everything it touches fits the LDS
 * staging area.  That area lists the block's own rows and then its external rows in ascending order
 * (neighbouring rows end up adjacent in LDS and in L2); in the run plan the external rows below the own
 * range come first and two zero rows last, so slots ascend with the column and a run never breaks at the
 * edge of the own range.  Returns 0 on success, -1 when out of memory, 1 when some 64-row slice references
 * more rows than fit the staging area or -- run plan, unless forced -- when the plan does not pay: zero fill
 * above 6 % of the plain SELL storage, or external rows above a quarter of the matrix stream. */
static int plan_staged(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl, scratch_t* s, int runs) {
  int ts = in->ts, m = in->m, ncols = m + in->halo;
  int cap_rows, blk_rows;
  if (runs) {
    /* panels of 16 columns: the plan is cut for 8 columns and a block is worked twice, once per half of the
     * panel (spmm.hip; staging area and pay-off test of stride 8).  One workgroup staging all 16 columns was
     * measured slower: 628 against 371 us, the LDS reads of 128 B per nonzero and lane dominate. */
    if (ts >= 16) ts /= 2;
    /* 8 columns: the rows of the staging area are 80 bytes apart (spmm.hip: spmm_row, no LDS bank conflicts) and a
     * workgroup may stage 80 KiB, two workgroups per CU.  Block rows / staging budget measured with the padded rows
     * (70^3, iterations/s at 8 | 16 columns): 192 / 60 KiB 1834 | 1038, 256 / 64 KiB 1776 | 977, **256 / 80 KiB
     * 1849 | 1094**, 320 / 80 KiB 1763 | 998, 320 / 100 KiB 1679 | 912 (before the padding: 192 rows / 48 KiB,
     * three workgroups per CU, 1832 | 1025). */
    cap_rows = (ts <= 4 ? 32768 : 81920) / (ts == 8 ? 80 : ts * 8) - 2;
    if (cap_rows > 65533) cap_rows = 65533;
    blk_rows = block_rows(in, 256, cap_rows);
  } else {
    /* LDS budget of a block: 32 KiB at ts <= 4, 64 KiB at ts = 8 (two workgroups per CU) */
    cap_rows = (ts <= 4 ? 32768 : 49152) / (ts * 8);
    if (cap_rows > 65535) cap_rows = 65535;
    /* 8-column panels: 192 rows and 48 KiB of staging (three workgroups per CU) measured 7 % faster */
    blk_rows = block_rows(in, ts <= 4 ? 256 : 192, cap_rows);
  }
  if (blk_rows < 64) return 1;
  if (cut_slices(in, pl, s)) return -1;
  int nslices = pl->nslices;
  size_t ns1 = (size_t)(nslices ? nslices : 1);
  const int* sl_row0 = ARR(pl, PA_PL_SL_ROW0, int);
  const int* sl_nrows = ARR(pl, PA_PL_SL_NROWS, int);
  size_t tot = (size_t)ARR(pl, PA_PL_SL_OFF, long long)[nslices];   /* entries of the plain SELL storage */
  double plain = (double)tot;
  int* blk_slice = ARR(pl, PA_PL_BLK_SLICE, int);
  int* blk_ext_off = (int*)arr_new(pl, PA_PL_BLK_EXT_OFF, ns1 + 1);
  int* blk_nlow = runs ? (int*)arr_new(pl, PA_PL_BLK_NLOW, ns1) : NULL;
  s->stamp = (int*)calloc(ncols ? ncols : 1, sizeof(int));
  s->slot_of = (int*)malloc((ncols ? ncols : 1) * sizeof(int));
  s->ext_cap = 1024;
  s->ent_cap = runs ? (size_t)(plain / 3.0 * 1.1) + 4096 : tot + 64;   /* runs: stored runs (64 per step of a slice) */
  if (!blk_ext_off || (runs && !blk_nlow) || !s->stamp || !s->slot_of || !arr_new(pl, PA_PL_EXT_ROWS, s->ext_cap) ||
      !arr_new(pl, PA_PL_COL16, s->ent_cap) || !arr_new(pl, PA_PL_VAL, s->ent_cap * (runs ? 3 : 1)))
    return -1;
  int nblk = 0, q = 0, max_stage = 0;
  while (q < nslices) {
    int nsl = 0;
    while (q + nsl < nslices && (nsl + 1) * 64 <= blk_rows) ++nsl;
    for (;;) {
      int r0 = sl_row0[q], r1 = sl_row0[q + nsl - 1] + sl_nrows[q + nsl - 1];
      int nown = r1 - r0, next, nlow;
      size_t mark0 = pl->a[PA_PL_EXT_ROWS].n;
      char h;
      if (collect_ext(in, pl, s, r0, r1, &next, &nlow, &h)) return -1;
      if (nown + next > cap_rows) {
        pl->a[PA_PL_EXT_ROWS].n = mark0;
        if (nsl == 1) return 1;
        nsl = (nsl + 1) / 2;
        continue;
      }
      if (!runs) nlow = 0;   /* the staged plan keeps all external rows behind the own rows */
      int* er = ARR(pl, PA_PL_EXT_ROWS, int) + mark0;
      sort_ints(er, next);
      for (int a = 0; a < next; ++a) s->slot_of[er[a]] = a < nlow ? a : nown + a;
      for (int sq = q; sq < q + nsl; ++sq) {
        if (!runs) fill_slots(in, pl, s, sq, r0, r1);
        else if (fill_runs(in, pl, s, sq, r0, r1, nlow)) return -1;
      }
      int stage = nown + next + (runs ? 2 : 0);
      if (stage > max_stage) max_stage = stage;
      blk_slice[nblk] = q; blk_ext_off[nblk] = (int)mark0; s->needs_halo[nblk] = h;
      if (runs) blk_nlow[nblk] = nlow;
      ++nblk;
      q += nsl;
      break;
    }
  }
  size_t next_tot = pl->a[PA_PL_EXT_ROWS].n;
  if (runs) {
    size_t nruns = pl->a[PA_PL_COL16].n, nr1 = nruns ? nruns : 1;
    double ext_bytes = (double)next_tot * ts * 8.0;
    if (in->want_runs < 2 && (3.0 * (double)nruns > 1.06 * plain || ext_bytes >= 0.25 * 10.0 * plain)) return 1;
    pl->stream_bytes = 26.0 * (double)nruns + 4.0 * (double)next_tot;
    pl->sell_entries = 3.0 * (double)nruns;
    pl->runs = 1; pl->runs_cols = ts;
    arr_set(pl, PA_PL_COL16, nruns, nr1);
    arr_set(pl, PA_PL_VAL, 3 * nruns, 3 * nr1);
    arr_set(pl, PA_PL_BLK_NLOW, (size_t)nblk, (size_t)(nblk > 0 ? nblk : 1));
  } else {
    for (size_t k = tot; k < tot + 64; ++k) { ARR(pl, PA_PL_COL16, unsigned short)[k] = 0; ARR(pl, PA_PL_VAL, double)[k] = 0.0; }
    pl->stream_bytes = 10.0 * (double)tot + 4.0 * (double)next_tot;
    pl->sell_entries = (double)tot;
    arr_set(pl, PA_PL_COL16, tot + 64, tot + 64);
    arr_set(pl, PA_PL_VAL, tot + 64, tot + 64);
  }
  if (finish_blocks(pl, s, nblk)) return -1;
  blk_ext_off[nblk] = (int)next_tot;
  arr_set(pl, PA_PL_BLK_EXT_OFF, (size_t)nblk + 1, (size_t)nblk + 1);
  arr_set(pl, PA_PL_EXT_ROWS, next_tot, next_tot + 1);   /* one spare entry: k_spmm_runs reads ids unconditionally */
  pl->staged = 1; pl->stage_cap = max_stage;
  return 0;
}

/* ------------------------------------------------------------- the choice ---- */
enum { FORM_WINDOW, FORM_STAGED, FORM_RUNS };

/* One attempt; whatever it leaves behind on a non-zero return is released here. */
static int attempt(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl, int form) {
  scratch_t s;
  memset(&s, 0, sizeof(s));
  int rc = form == FORM_WINDOW ? plan_window(in, pl, &s) : plan_staged(in, pl, &s, form == FORM_RUNS);
  scratch_free(&s);
  if (rc) {
    size_t oom = pl->oom_entries;
    pa_spmm_plan_free(pl);
    pl->oom_entries = oom;
  }
  return rc;
}

int pa_spmm_plan_build(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl) {
  memset(pl, 0, sizeof(*pl));
  /* -1 (default): stage when the external rows a block copies are small next to its matrix
   * slice (long rows: elasticity); short rows (7-point stencils) gather through L2 instead */
  int want = in->want_staged, ts = in->ts, rc;
  if (want != 0 && in->want_runs) {
    /* rows whose nonzeros come in runs of consecutive columns (vector problems: 3 dofs per
     * node) share one LDS slot per run of three: 8.67 B per nonzero instead of 10 */
    rc = attempt(in, pl, FORM_RUNS);
    if (rc <= 0) return rc;
  }
  if (want < 0 && ts >= 16) want = 0; /* wide panels: the 128-B X rows gather well from L2 (measured) */
  if (want != 0) {
    rc = attempt(in, pl, FORM_STAGED);
    if (rc < 0) return rc;
    if (rc == 0) {
      double ext_bytes = (pl->stream_bytes - 10.0 * pl->sell_entries) / 4.0 * ts * 8.0;
      /* round 4: at up to 4 columns the staged kernel (batched staging, its Gram block in the epilogue) is worth
       * it up to external rows of half the matrix slice: 7-point Poisson 100^3 (38 %) 226.6 -> 221.6 us per
       * iteration against the window kernel, although the plain product alone is 3 us slower
       * (tools/probe/r4_poisson_plan_ab.py); wider panels keep the quarter */
      const double thr = ts <= 4 ? 0.5 : 0.25;
      if (want > 0 || ext_bytes < thr * 10.0 * pl->sell_entries) return 0;
      pa_spmm_plan_free(pl); /* not worth it: use the general kernel */
    }
  }
  return attempt(in, pl, FORM_WINDOW);
}

/* ---------------------------------------------------------- the value map ---- */
int pa_spmm_plan_value_map(const pa_spmm_plan_in_t* in, pa_spmm_value_map_t* vm) {
  memset(vm, 0, sizeof(*vm));
  const size_t nnz = (size_t)in->rowPtr[in->m];
  double* code = (double*)pa_big_alloc((nnz ? nnz : 1) * sizeof(double));
  if (!code) return -1;
  for (size_t k = 0; k < nnz; ++k) code[k] = (double)(k + 1);
  pa_spmm_plan_in_t coded = *in;
  coded.val = code;
  pa_spmm_host_plan_t pl;
  int rc = pa_spmm_plan_build(&coded, &pl);
  free(code);
  if (rc) return -1;
  const size_t n = pl.a[PA_PL_VAL].n;
  const double* v = ARR(&pl, PA_PL_VAL, double);
  uint32_t* map = (uint32_t*)pa_big_alloc((n ? n : 1) * sizeof(uint32_t));
  if (!map) { pa_spmm_plan_free(&pl); return -1; }
  for (size_t s = 0; s < n; ++s) map[s] = (uint32_t)v[s];
  vm->map = map; vm->n = n;
  vm->nslices = pl.nslices; vm->nblk = pl.nblk; vm->staged = pl.staged; vm->runs = pl.runs; vm->runs_cols = pl.runs_cols;
  pa_spmm_plan_free(&pl);
  return 0;
}
