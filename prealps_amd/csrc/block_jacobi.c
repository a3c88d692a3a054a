/*
 * block_jacobi.c -- block-Jacobi preconditioner Z = blockdiag(A)^-1 X with one
 * exact SPD solve per subdomain, factors resident in HBM.
 *
 * Reference behaviour kept (under /root/reference):
 *   preAlps_BlockJacobiCreate  src/preconditioners/block_jacobi.c:26-63
 *       diagonal block of the local row panel = entries whose column lies in
 *       the part's own row range (utils/cplm_v0/cplm_v0_matcsr.c:287-463),
 *       Cholesky factorisation (PARDISO phase 12, cplm_kernels.c:741-784)
 *   preAlps_BlockJacobiApply   block_jacobi.c:93-109 -> PARDISO phase 33 with
 *       nrhs = A_in->info.n (cplm_kernels.c:790-853)
 *   preAlps_BlockJacobiFree    block_jacobi.c:111-118
 *
 * MI355X design: a sparse direct solver with supernodes and pivoting queues
 * does not map onto 64-wide wavefronts; instead every block is reordered by
 * reverse Cuthill-McKee, factored once as a dense-band Cholesky L L^T (exact:
 * no fill leaves the band) and stored twice, column-wise for the forward sweep
 * and row-wise (reversed) for the backward sweep, so both sweeps stream their
 * band with coalesced loads (bj_band.hip: k_bj_apply).  One process owns
 * nparts/size blocks; one wavefront solves one block.
 *
 * This unit: the state, the device side of the create, the apply.  The host work of the create and the layout
 * table are bj_build.c's (pure host code), the refresh in place is bj_update.c's, the coarse space bj_coarse.c's;
 * bj_priv.h is what the three share.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_priv.h"

static pa_bj_t g_bj;
pa_bj_t* pa_bj_state(void) { return &g_bj; }
static double g_bj_setup_s[2];
double pa_bj_setup_seconds(int which) { return g_bj_setup_s[which ? 1 : 0]; }

double pa_bj_factor_bytes(void) { return g_bj.created ? g_bj.factor_bytes : 0.0; }
static int g_bj_values_epoch;   /* pa_operator_values_epoch() at the last create: a smaller one than the operator's means a lagged factor */
int pa_bj_values_epoch(void) { return g_bj_values_epoch; }
void pa_bj_values_epoch_sync(void) { g_bj_values_epoch = pa_operator_values_epoch(); }
int pa_bj_max_bandwidth(void) { return g_bj.created ? g_bj.lay.max_bw : 0; }
int pa_bj_nparts(void) { return g_bj.created ? g_bj.np : 0; }
int pa_bj_nd_blocks(void) { return g_bj.created ? g_bj.nd_blocks : 0; }
int pa_bj_nd_precision(void) { return g_bj.created && g_bj.nd_blocks > 0 ? pa_nd_precision() : 0; }

/* Storage of the sparse factors of the next creates: 64 / 32 bits, 0 = PREALPS_BJ_ND_PRECISION (band blocks: fp64) */
static int g_nd_bits = 0;
int preAlps_hip_set_nd_precision(int bits) {
  if (bits != 0 && bits != 32 && bits != 64)
    return PA_FAIL("precision %d refused: 64 (double), 32 (single) or 0 (follow PREALPS_BJ_ND_PRECISION)", bits);
  g_nd_bits = bits;
  return 0;
}
/* storage of the one-copy band records of bj_g4.hip (64 / 32), 0 if no class has them */
int pa_bj_band_precision(void) { return g_bj.created && g_bj.d_Lg4 ? g_bj.g4_bits : 0; }

/* Storage of the one-copy band records of the next creates: 64 / 32 bits, 0 = PREALPS_BJ_BAND_PRECISION.
 * Independent of preAlps_hip_set_nd_precision. */
static int g_band_bits = 0;
int preAlps_hip_set_band_precision(int bits) {
  if (bits != 0 && bits != 32 && bits != 64)
    return PA_FAIL("precision %d refused: 64 (double), 32 (single) or 0 (follow PREALPS_BJ_BAND_PRECISION)", bits);
  g_band_bits = bits;
  return 0;
}
double pa_bj_pairs_bytes(void) { return g_bj.created ? g_bj.pairs_bytes : 0.0; }
double pa_bj_g4_bytes(void) { return g_bj.created ? g_bj.g4_bytes : 0.0; }
/* blocks of the apply when it can leave the ECG Gram block [in | prev]^T out behind (pa_k_bj_gram_arm): every
 * local block in one class served by bj_g4.hip, no sparse-factored blocks; 0: it cannot */
int pa_bj_gram_blocks(void) {
  const pa_bj_t* s = &g_bj;
  const pa_bj_layout_t* L = &s->lay;
  if (!s->created || s->nd_blocks > 0 || !s->d_Lg4 || L->nclass != 1 || !L->class_g4[0] || L->class_count[0] != s->np) return 0;
  if (s->co.on) return 0;      /* the coarse correction changes `out` after the block solve: its Gram block would be stale */
  return s->np;
}

/* + 1 whenever what preAlps_BlockJacobiApply launches or the device arrays it reads change: a create, a free, a coarse
 * space set, replaced, cleared or dropped.  A solver that replays captured iteration segments (ecg.c: seg_begin)
 * compares it and captures anew: its graphs hold the old launches and the old pointers. */
static int g_bj_apply_epoch;
int pa_bj_apply_epoch(void) { return g_bj_apply_epoch; }
void pa_bj_apply_epoch_bump(void) { ++g_bj_apply_epoch; }

void preAlps_BlockJacobiFree(void) {
  pa_bj_t* s = &g_bj;
  pa_bj_coarse_release(&s->co);
  ++g_bj_apply_epoch;
  pa_rt_free(s->d_row0); pa_rt_free(s->d_nrows); pa_rt_free(s->d_bw); pa_rt_free(s->d_off);
  pa_rt_free(s->d_map_f); pa_rt_free(s->d_map_b);
  pa_rt_free(s->d_Lf); pa_rt_free(s->d_Lb); pa_rt_free(s->d_invd_f); pa_rt_free(s->d_invd_b);
  pa_rt_free(s->d_Lf2); pa_rt_free(s->d_Lb2); pa_rt_free(s->d_off2); pa_rt_free(s->d_Lg4);
  pa_rt_free(s->d_off_read); pa_rt_free(s->d_off2_read); pa_rt_free(s->d_rep); pa_rt_free(s->d_share_list); pa_rt_free(s->d_share_cnt);
  free(s->h_rep);
  for (int c = 0; c < PA_BJ_MAX_CLASSES; ++c) { pa_rt_free(s->d_class_list[c]); pa_rt_free(s->d_ptask[c]); }
  pa_bj_layout_free(&s->lay);
  free(s->h_row0); free(s->h_nrows); free(s->h_bw); free(s->h_grow0); free(s->h_map_f); free(s->h_is_nd);
  pa_rt_free(s->d_bm_src); pa_rt_free(s->d_bm_dst); pa_rt_free(s->d_bm_chunk_blk); pa_rt_free(s->d_bm_chunk_first);
  pa_rt_free(s->d_boff); pa_rt_free(s->d_slist); pa_rt_free(s->d_blist); pa_rt_free(s->d_fail);
  pa_nd_free();
  memset(s, 0, sizeof(*s));
}

/* ---- creation: the switches, then one stage per step ------------------------- */
/* The stages report as the entry point they belong to: the error texts name preAlps_BlockJacobiCreate. */
#define BJ_FAIL(...) pa_fail_at("preAlps_BlockJacobiCreate", __VA_ARGS__)

/* The switches of a create, read once. */
typedef struct {
  int nd_bits, band_bits;     /* storage of the sparse factors / of the one-copy band records */
  int nd_mode, nd_rows;       /* PREALPS_BJ_ND, PREALPS_BJ_ND_ROWS */
  int dev_factor;             /* PREALPS_BJ_FACTOR != host */
  int wide_from;              /* PREALPS_BJ_WIDE_FROM, negative: absent */
  int want_g4, want_pairs;    /* PREALPS_BJ_G4 / PREALPS_BJ_PAIRS != 0 */
  int share;                  /* PREALPS_BJ_SHARE != 0: identical blocks read one block's records (bj_share.h) */
  int pair;                   /* PREALPS_BJ_PAIR: 0 never two blocks per wavefront, 1 whenever a list has a pair, -1 (unset): the rule */
} bj_switches_t;

/* Storage bits of a factor: the value set through the API, else the switch `name` (double / single). */
static int bj_storage_bits(int set, const char* name, const char* what, int* bits) {
  const char* pe = getenv(name);
  if (set) *bits = set;
  else if (!pe || !*pe || !strcmp(pe, "double")) *bits = 64;
  else if (!strcmp(pe, "single")) *bits = 32;
  else return BJ_FAIL("%s=%s: expected double or single (storage of the %s)", name, pe, what);
  return 0;
}

static int bj_read_switches(bj_switches_t* sw) {
  /* band blocks stay fp64 but for the one-copy records of bj_g4.hip */
  if (bj_storage_bits(g_nd_bits, "PREALPS_BJ_ND_PRECISION", "sparse block factors", &sw->nd_bits) ||
      bj_storage_bits(g_band_bits, "PREALPS_BJ_BAND_PRECISION", "one-copy band records", &sw->band_bits))
    return 1;
  /* Large blocks (few subdomains of thousands of rows, the reference's own regime) get a sparse
   * nested-dissection factor instead of a band (nd.c).  PREALPS_BJ_ND: 0 never, 1 (default) for
   * blocks of at least PREALPS_BJ_ND_ROWS (2048) rows whose band exceeds 256, 2 for every block of
   * at least PREALPS_BJ_ND_ROWS rows.  (Measured on elasticity 70^3, per apply: blocks of 17.5 k rows
   * 2.3 ms against 15.3 ms with the band kernels; 2187 rows 1.35 against 1.46 ms; 648 rows 0.90
   * against 0.60 ms: small blocks stay with the band.) */
  sw->nd_mode = getenv("PREALPS_BJ_ND") ? atoi(getenv("PREALPS_BJ_ND")) : 1;
  sw->nd_rows = getenv("PREALPS_BJ_ND_ROWS") ? atoi(getenv("PREALPS_BJ_ND_ROWS")) : 2048;
  /* PREALPS_BJ_FACTOR=host keeps every factorisation on the host threads */
  const char* fenv = getenv("PREALPS_BJ_FACTOR");
  sw->dev_factor = !(fenv && !strcmp(fenv, "host"));
  /* PREALPS_BJ_WIDE_FROM = first band that is NOT given to a single wavefront, minus one (tests use it to reach
   * both dispatches on small problems); the layout clamps it, a negative value like any other below its range */
  const char* e = getenv("PREALPS_BJ_WIDE_FROM");
  sw->wide_from = -1;
  if (e && *e) { sw->wide_from = atoi(e); if (sw->wide_from < 0) sw->wide_from = 0; }
  sw->want_g4 = !(getenv("PREALPS_BJ_G4") && atoi(getenv("PREALPS_BJ_G4")) == 0);
  sw->want_pairs = !(getenv("PREALPS_BJ_PAIRS") && atoi(getenv("PREALPS_BJ_PAIRS")) == 0);
  sw->share = !(getenv("PREALPS_BJ_SHARE") && atoi(getenv("PREALPS_BJ_SHARE")) == 0);
  const char* pe = getenv("PREALPS_BJ_PAIR");
  sw->pair = pe && *pe ? (atoi(pe) != 0) : -1;
  return 0;
}

/* ---- stage 1b: the classes of identical blocks (bj_share.h) -------------------- */
/* Before the bands are handed on: a narrow block whose band is assembled row-major may read the records of the
 * lowest-numbered block with the same rows, bandwidth and band bytes (with PREALPS_BJ_FACTOR=host the bands hold
 * the factor: identical factors share as well).  Wide / entry-list blocks and sparse-factored blocks read their
 * own.  share == 0 (PREALPS_BJ_SHARE=0): every block its own. */
static int bj_share_pass(pa_bj_t* s, const pa_bj_build_t* B, int share) {
  const int np = B->np;
  const double t0 = pa_wtime();
  s->h_rep = (int*)malloc((size_t)(np ? np : 1) * sizeof(int));
  char* el = (char*)malloc((size_t)(np ? np : 1));
  if (!s->h_rep || !el) { free(el); return BJ_FAIL("out of host memory for the classes of %d blocks", np); }
  for (int p = 0; p < np; ++p) el[p] = share && !B->is_nd[p] && B->bands[p] && B->bw[p] <= s->lay.wide_from;
  const pa_bj_share_in_t in = {.np = np, .nrows = B->nrows, .bw = B->bw, .eligible = el, .bands = B->bands,
                               .threads = pa_host_threads(), .hash_mask = ~0ull};
  const int rc = pa_bj_share_classes(&in, s->h_rep, &s->share_classes);
  free(el);
  if (rc) return BJ_FAIL("out of host memory for the classes of %d blocks", np);
  s->share_on = share; s->share_members = 0; s->shared_elems2 = 0;
  for (int p = 0; p < np; ++p)
    if (s->h_rep[p] != p) { ++s->share_members; s->shared_elems2 += 8LL * ((B->nrows[p] + 7) / 8) * (B->bw[p] + 4); }
  s->shared_blocks = s->share_members;
  s->share_s = pa_wtime() - t0;
  if (getenv("PREALPS_SETUP_TRACE"))
    fprintf(stderr, "[setup] block classes (%d of %d blocks share, %d classes)  %.3f s\n", s->share_members, np,
            s->share_classes, s->share_s);
  return 0;
}

/* The read offsets on the device, and what the refresh's k_bj_share_check needs: rep and the list of the blocks
 * that read another block's records. */
static int bj_upload_share(pa_bj_t* s) {
  const int np = s->np, nm = s->share_members;
  const size_t np1 = (size_t)np + 1;
  const pa_bj_layout_t* L = &s->lay;
  long long* h = (long long*)malloc(2 * np1 * sizeof(long long));
  int* list = (int*)malloc((size_t)(nm ? nm : 1) * sizeof(int));
  int rc = 0, x = 0;
  if (!h || !list) { free(h); free(list); return BJ_FAIL("out of host memory for the read offsets of %d blocks", np); }
  for (int p = 0; p < np; ++p) {
    h[p] = L->off[s->h_rep[p]]; h[np1 + p] = L->off2[s->h_rep[p]];
    if (s->h_rep[p] != p) list[x++] = p;
  }
  /* (Up to 8 -- and 64 -- members of a class as own readers, the others spread over them round-robin, against
   * contention for the L2 channels of one record: measured, no gain -- DESIGN.md section 4p.) */
  h[np] = L->off[np]; h[np1 + np] = L->off2[np];
  s->d_off_read = (long long*)pa_rt_malloc(np1 * sizeof(long long));
  if (s->d_off2) s->d_off2_read = (long long*)pa_rt_malloc(np1 * sizeof(long long));
  s->d_rep = (int*)pa_rt_malloc((size_t)(np ? np : 1) * sizeof(int));
  s->d_share_list = (int*)pa_rt_malloc((size_t)(nm ? nm : 1) * sizeof(int));
  s->d_share_cnt = (unsigned long long*)pa_rt_malloc(2 * sizeof(unsigned long long));
  if (!s->d_off_read || (s->d_off2 && !s->d_off2_read) || !s->d_rep || !s->d_share_list || !s->d_share_cnt ||
      pa_rt_h2d(s->d_off_read, h, np1 * sizeof(long long)) ||
      (s->d_off2 && pa_rt_h2d(s->d_off2_read, h + np1, np1 * sizeof(long long))) ||
      pa_rt_h2d(s->d_rep, s->h_rep, (size_t)np * sizeof(int)) || pa_rt_h2d(s->d_share_list, list, (size_t)nm * sizeof(int)))
    rc = BJ_FAIL("uploading the read offsets failed: %s", pa_rt_error());
  free(h); free(list);
  return rc;
}

/* ---- stage 8b: the pair tasks of the classes of the layout that bj_g4.hip serves ---- */
/* Behind the class pass and the second layouts: for every class of the layout with fp64 one-copy records, the tasks
 * (i0, i1) of its launch list (bj_share.h), built once and uploaded once.  Whether a launch takes them is the launch
 * planner's rule (bj_g4_plan.c); with no sharing every block is a class of one and no list has a pair. */
static int bj_pair_pass(pa_bj_t* s, int pair_mode) {
  const pa_bj_layout_t* L = &s->lay;
  int rc = 0;
  s->pair_mode = pair_mode; s->pair_tasks = 0; s->paired_blocks = 0;
  if (!s->d_Lg4 || s->g4_bits != 64 || s->share_members == 0) return 0;
  for (int c = 0; c < L->nclass && !rc; ++c) {
    const int count = L->class_count[c];
    if (!L->class_g4[c] || count < 2) continue;
    int* tasks = (int*)malloc(2 * (size_t)count * sizeof(int));
    int nt = 0, paired = 0;
    if (!tasks || pa_bj_pair_tasks(s->np, L->class_list[c], count, s->h_rep, s->h_nrows, s->h_bw, tasks, &nt, &paired)) {
      free(tasks);
      return BJ_FAIL("out of host memory for the pair tasks of %d blocks", count);
    }
    if (paired > 0) {
      s->d_ptask[c] = (int*)pa_rt_malloc(2 * (size_t)nt * sizeof(int));
      if (!s->d_ptask[c] || pa_rt_h2d(s->d_ptask[c], tasks, 2 * (size_t)nt * sizeof(int)))
        rc = BJ_FAIL("uploading the pair tasks failed: %s", pa_rt_error());
      s->class_ptask[c].tasks = s->d_ptask[c]; s->class_ptask[c].ntasks = nt; s->class_ptask[c].paired = paired;
      s->pair_tasks += nt; s->paired_blocks += paired;
    }
    free(tasks);
  }
  if (getenv("PREALPS_SETUP_TRACE"))
    fprintf(stderr, "[setup] pair tasks (%d tasks, %d of %d blocks have a partner)\n", s->pair_tasks, s->paired_blocks, s->np);
  return rc;
}

/* ---- stage 2: the device arrays of the records ----------------------------------- */
/* They come first: the factors are written in place, by the factorisation kernel for the blocks the device
 * factors and by staged uploads for the ones factored on the host. */
static int bj_alloc_records(pa_bj_t* s) {
  const size_t m = (size_t)s->m, tot = s->lay.tot, pad = s->lay.pad;
  s->d_invd_f = (double*)pa_rt_malloc((m ? m : 1) * sizeof(double));
  s->d_invd_b = (double*)pa_rt_malloc((m ? m : 1) * sizeof(double));
  s->d_Lf = (double*)pa_rt_malloc((tot + pad) * sizeof(double));
  s->d_Lb = (double*)pa_rt_malloc((tot + pad) * sizeof(double));
  if (!s->d_Lf || !s->d_Lb || !s->d_invd_f || !s->d_invd_b ||
      pa_rt_memset(s->d_Lf, 0, (tot + pad) * sizeof(double)) || pa_rt_memset(s->d_Lb, 0, (tot + pad) * sizeof(double)))
    return BJ_FAIL("allocating %zu factor entries on the device failed: %s", tot, pa_rt_error());
  return 0;
}

/* ---- stage 3: records of the host-factored blocks, staged upload ------------ */
/* Host-factored blocks: runs of consecutive blocks (up to 64 MiB of records) are laid out
 * by the host threads into a staging buffer (256 MiB, or one block if larger) and go to
 * the device in one copy each.  Then 1 / L(j,j) of every row (the device factorisation overwrites its own). */
static int bj_layout_host(pa_bj_t* s, pa_bj_build_t* B) {
  const int np = B->np;
  const pa_bj_layout_t* L = &s->lay;
  const long long* off = L->off;
  const size_t cap = (size_t)32 << 20;                   /* doubles: 256 MiB per staging buffer */
  size_t sf_cap = 0;
  double* sf = NULL; double* sg = NULL;
  int rc = 0, q = 0;
  while (L->ndev + L->nnd < np && q < np && !rc) {
    if (s->dev_factor || B->is_nd[q]) { ++q; continue; }
    int q1 = q;
    while (q1 < np && !s->dev_factor && !B->is_nd[q1] && (q1 == q || (size_t)(off[q1 + 1] - off[q]) <= cap)) ++q1;
    size_t len = (size_t)(off[q1] - off[q]);
    if (len > sf_cap) {
      sf_cap = len;
      sf = (double*)realloc(sf, sf_cap * sizeof(double));
      sg = (double*)realloc(sg, sf_cap * sizeof(double));
      if (!sf || !sg) { rc = BJ_FAIL("out of host memory for %zu factor entries", sf_cap); break; }
    }
    memset(sf, 0, len * sizeof(double));
    memset(sg, 0, len * sizeof(double));
    /* work items = slabs of 256 steps of one block, so that a run of few large blocks
     * still keeps every host thread busy */
    int nitem = 0;
    for (int x = q; x < q1; ++x) nitem += (B->nrows[x] + 255) / 256;
    int* item_part = (int*)malloc((nitem ? nitem : 1) * sizeof(int));
    int* item_j0 = (int*)malloc((nitem ? nitem : 1) * sizeof(int));
    if (!item_part || !item_j0) { free(item_part); free(item_j0); rc = BJ_FAIL("out of host memory for %d slabs", nitem); break; }
    nitem = 0;
    for (int x = q; x < q1; ++x)
      for (int j0 = 0; j0 < B->nrows[x]; j0 += 256) { item_part[nitem] = x; item_j0[nitem++] = j0; }
#pragma omp parallel for num_threads(pa_host_threads()) schedule(dynamic, 4)
    for (int it = 0; it < nitem; ++it) {
      const int x = item_part[it];
      pa_bj_layout_slab(B, L->wide_from, x, item_j0[it], sf + (off[x] - off[q]), sg + (off[x] - off[q]));
    }
    free(item_part); free(item_j0);
    if (pa_rt_h2d(s->d_Lf + off[q], sf, len * sizeof(double)) || pa_rt_h2d(s->d_Lb + off[q], sg, len * sizeof(double)))
      rc = BJ_FAIL("uploading the block factors failed: %s", pa_rt_error());
    q = q1;
  }
  free(sf); free(sg);
  if (!rc && (pa_rt_h2d(s->d_invd_f, B->invd_f, (size_t)B->m * sizeof(double)) ||
              pa_rt_h2d(s->d_invd_b, B->invd_b, (size_t)B->m * sizeof(double))))
    rc = BJ_FAIL("uploading the block factors failed: %s", pa_rt_error());
  return rc;
}

/* ---- stage 4: the block lists of the layout's classes on the device ---------- */
static int bj_upload_classes(pa_bj_t* s) {
  const pa_bj_layout_t* L = &s->lay;
  int rc = 0;
  for (int c = 0; c < L->nclass && !rc; ++c) {
    const size_t bytes = (size_t)L->class_count[c] * sizeof(int);
    s->d_class_list[c] = (int*)pa_rt_malloc(bytes);
    rc = !s->d_class_list[c] || pa_rt_h2d(s->d_class_list[c], L->class_list[c], bytes);
    s->class_list_c[c] = s->d_class_list[c];
  }
  if (rc) rc = BJ_FAIL("uploading block lists failed: %s", pa_rt_error());
  return rc;
}

/* ---- stage 5: the per-block and per-row index arrays ------------------------ */
static int bj_upload_index(pa_bj_t* s, const pa_bj_build_t* B) {
  const int np = B->np, m = B->m;
  s->d_row0 = (int*)pa_rt_malloc(np * sizeof(int));
  s->d_nrows = (int*)pa_rt_malloc(np * sizeof(int));
  s->d_bw = (int*)pa_rt_malloc(np * sizeof(int));
  s->d_off = (long long*)pa_rt_malloc((np + 1) * sizeof(long long));
  s->d_map_f = (int*)pa_rt_malloc((size_t)(m ? m : 1) * sizeof(int));
  s->d_map_b = (int*)pa_rt_malloc((size_t)(m ? m : 1) * sizeof(int));
  int bad = !s->d_row0 || !s->d_nrows || !s->d_bw || !s->d_off || !s->d_map_f || !s->d_map_b;
  bad = bad || pa_rt_h2d(s->d_row0, B->row0, np * sizeof(int)) || pa_rt_h2d(s->d_nrows, B->nrows, np * sizeof(int)) ||
        pa_rt_h2d(s->d_bw, B->bw, np * sizeof(int)) || pa_rt_h2d(s->d_off, s->lay.off, (np + 1) * sizeof(long long)) ||
        pa_rt_h2d(s->d_map_f, B->map_f, (size_t)m * sizeof(int)) || pa_rt_h2d(s->d_map_b, B->map_b, (size_t)m * sizeof(int));
  return bad ? BJ_FAIL("uploading the block factors failed: %s", pa_rt_error()) : 0;
}

/* ---- stage 6: factorisation on the device ------------------------------------ */
/* Narrow bands: runs of consecutive blocks go up in one copy of at most 256 MiB, and the host copy of a
 * band is released as soon as it is on the device. */
static int bj_upload_bands(pa_bj_build_t* B, const long long* boff, double* d_band) {
  const int np = B->np;
  const size_t cap = (size_t)32 << 20;
  double* hb = NULL;
  size_t hb_cap = 0;
  int rc = 0;
  for (int q = 0; q < np && !rc; ) {
    if (!B->bands[q]) { ++q; continue; }
    int q1 = q + 1;
    while (q1 < np && B->bands[q1] && (size_t)(boff[q1 + 1] - boff[q]) <= cap) ++q1;
    size_t len = (size_t)(boff[q1] - boff[q]);
    if (len > hb_cap) { hb_cap = len; hb = (double*)realloc(hb, hb_cap * sizeof(double)); }
    if (!hb) { rc = BJ_FAIL("out of host memory for %zu band entries", len); break; }
#pragma omp parallel for num_threads(pa_host_threads()) schedule(dynamic, 16)
    for (int x = q; x < q1; ++x)
      memcpy(hb + (boff[x] - boff[q]), B->bands[x], (size_t)B->nrows[x] * (B->bw[x] + 1) * sizeof(double));
    if (pa_rt_h2d(d_band + boff[q], hb, len * sizeof(double))) rc = BJ_FAIL("uploading the bands failed: %s", pa_rt_error());
    for (int x = q; x < q1; ++x) { free(B->bands[x]); B->bands[x] = NULL; }
    q = q1;
  }
  free(hb);
  return rc;
}

/* Wide bands (d_band zeroed): only their entries are shipped, gathered into one list, and scattered on
 * the device (k_scatter). */
static int bj_scatter_wide(const pa_bj_build_t* B, const long long* boff, double* d_band) {
  const int np = B->np;
  int rc = 0;
  size_t ntot = 0;
  size_t* cbase = (size_t*)malloc(((size_t)np + 1) * sizeof(size_t));
  for (int q = 0; q < np && cbase; ++q) { cbase[q] = ntot; ntot += B->coo_n[q]; }
  long long* go = (long long*)malloc((ntot ? ntot : 1) * sizeof(long long));
  double* gv = (double*)malloc((ntot ? ntot : 1) * sizeof(double));
  long long* d_go = (long long*)pa_rt_malloc((ntot ? ntot : 1) * sizeof(long long));
  double* d_gv = (double*)pa_rt_malloc((ntot ? ntot : 1) * sizeof(double));
  if (!cbase || !go || !gv || !d_go || !d_gv) rc = BJ_FAIL("out of memory for %zu band entries", ntot);
  if (!rc) {
#pragma omp parallel for num_threads(pa_host_threads()) schedule(dynamic, 1)
    for (int q = 0; q < np; ++q)
      for (size_t e = 0; e < B->coo_n[q]; ++e) { go[cbase[q] + e] = boff[q] + B->coo_off[q][e]; gv[cbase[q] + e] = B->coo_val[q][e]; }
    if (pa_rt_h2d(d_go, go, ntot * sizeof(long long)) || pa_rt_h2d(d_gv, gv, ntot * sizeof(double)) ||
        pa_k_scatter(ntot, d_go, d_gv, d_band) || pa_rt_sync())
      rc = BJ_FAIL("assembling the wide bands on the device failed: %s", pa_rt_error());
  }
  pa_rt_free(d_go); pa_rt_free(d_gv); free(go); free(gv); free(cbase);
  return rc;
}

int pa_bj_factor_launch(const pa_bj_t* s, const int* d_slist, const int* d_blist, const long long* d_boff,
                        double* d_band, int* d_fail, int* fail) {
  const pa_bj_layout_t* L = &s->lay;
  return pa_k_bj_factor(d_slist, L->ns, L->wsmall, s->d_row0, s->d_nrows, s->d_bw, s->d_off, d_boff, d_band, s->d_Lf,
                        s->d_Lb, s->d_invd_f, s->d_invd_b, d_fail) ||
         pa_k_bj_factor_big(d_blist, L->nbig, L->wbig, L->wide_from, s->d_row0, s->d_nrows, s->d_bw, s->d_off, d_boff,
                            d_band, s->d_Lf, s->d_Lb, s->d_invd_f, s->d_invd_b, d_fail) ||
         pa_rt_d2h(fail, d_fail, sizeof(int));
}

int pa_bj_fail_global_row(int row_off, const int* map_f, const int* row0, const int* nrows, int np, int fail) {
  const int pos = fail - 1;       /* local (factor-order) position; q: the block that holds it */
  int q = 0;
  for (int x = 0; x < np; ++x) if (pos >= row0[x] && pos < row0[x] + nrows[x]) { q = x; break; }
  return row_off + map_f[pos] + row0[q];
}

/* Ship the assembled bands, factor and lay out on the device: bands up to dev_wmax with
 * the LDS-window kernel (row-major band), wider ones with the blocked kernel
 * (diagonal-major band, factored in place). */
static int bj_factor_device(pa_bj_t* s, pa_bj_build_t* B) {
  const int np = B->np;
  const pa_bj_layout_t* L = &s->lay;
  const size_t btot = L->btot;
  int rc = 0;
  double* d_band = (double*)pa_rt_malloc((btot ? btot : 1) * sizeof(double));
  long long* d_boff = (long long*)pa_rt_malloc((np + 1) * sizeof(long long));
  int* d_slist = (int*)pa_rt_malloc((L->ns ? L->ns : 1) * sizeof(int));
  int* d_blist = (int*)pa_rt_malloc((L->nbig ? L->nbig : 1) * sizeof(int));
  int* d_fail = (int*)pa_rt_malloc(sizeof(int));
  int fail = 0;
  if (!d_band || !d_boff || !d_slist || !d_blist || !d_fail)
    rc = BJ_FAIL("allocating %zu band entries on the device failed: %s", btot, pa_rt_error());
  const int tr = getenv("PREALPS_SETUP_TRACE") != NULL;
  double t_tr = pa_wtime();
  if (!rc && L->nbig > 0 && pa_rt_memset(d_band, 0, btot * sizeof(double))) rc = BJ_FAIL("%s", pa_rt_error());
  if (!rc) rc = bj_upload_bands(B, L->boff, d_band);
  if (!rc && L->nbig > 0) rc = bj_scatter_wide(B, L->boff, d_band);
  if (tr) { fprintf(stderr, "[setup] band upload (%.1f GB)        %.3f s\n", 8e-9 * (double)btot, pa_wtime() - t_tr); t_tr = pa_wtime(); }
  if (!rc) {
    if (pa_rt_h2d(d_boff, L->boff, (np + 1) * sizeof(long long)) || pa_rt_h2d(d_slist, L->slist, L->ns * sizeof(int)) ||
        pa_rt_h2d(d_blist, L->blist, L->nbig * sizeof(int)) || pa_rt_h2d(d_fail, &fail, sizeof(int)) ||
        pa_bj_factor_launch(s, d_slist, d_blist, d_boff, d_band, d_fail, &fail))
      rc = BJ_FAIL("factorising the diagonal blocks on the device failed: %s", pa_rt_error());
    else if (fail > 0)
      rc = BJ_FAIL("diagonal block is not SPD (global row %d)",
                   pa_bj_fail_global_row(s->row_off, B->map_f, B->row0, B->nrows, np, fail));
  }
  if (tr) fprintf(stderr, "[setup] device factorisation + layout  %.3f s\n", pa_wtime() - t_tr);
  pa_rt_free(d_band); pa_rt_free(d_boff); pa_rt_free(d_slist); pa_rt_free(d_blist); pa_rt_free(d_fail);
  return rc;
}

/* ---- stage 7: the sparse-factored blocks go to nd.c -------------------------- */
int pa_bj_nd_handoff(const char* who, const CPLM_Mat_CSR_t* A, int np, const char* is_nd, int nnd, const int* row0,
                     const int* nrows, const int* grow0, int m, int bits, int row_off) {
  int* ndl = (int*)malloc((size_t)(nnd ? nnd : 1) * sizeof(int));
  int x = 0, nd_fail = -1, rc = 0;
  if (!ndl) return pa_fail_at(who, "out of host memory");
  for (int q = 0; q < np; ++q) if (is_nd[q]) ndl[x++] = q;
  const int r2 = pa_nd_create(A, nnd, ndl, row0, nrows, grow0, m, bits, &nd_fail);
  if (r2 == 2) rc = pa_fail_at(who, "diagonal block is not SPD (global row %d)", row_off + nd_fail);
  else if (r2) rc = 1;
  free(ndl);
  return rc;
}

/* ---- stage 8: second layouts -------------------------------------------------- */
/* tot2 elements of 8 or 4 bytes (off2 counts elements: every offset a multiple of 8 of them, so a block
 * starts 32-byte aligned in fp32 too), and 8 KiB of zeroed slack: a request of the apply reads whole KiB
 * from a chunk's start, up to 1 KiB beyond the end of the last block's last chunk. */
int pa_bj_launch_g4(const pa_bj_t* s) {
  const pa_bj_layout_t* L = &s->lay;
  for (int c = 0; c < L->nclass; ++c)
    if (L->class_g4[c] &&
        (s->g4_bits == 32
           ? pa_k_bj_g4_setup_f32(s->d_class_list[c], L->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lf, (float*)s->d_Lg4)
           : pa_k_bj_g4_setup(s->d_class_list[c], L->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lf, (double*)s->d_Lg4)))
      return 1;
  return 0;
}

int pa_bj_launch_pairs(const pa_bj_t* s) {
  const pa_bj_layout_t* L = &s->lay;
  for (int c = 0; c < L->nclass; ++c)
    if (L->class_pairs[c])
      if (pa_k_bj_pairs(s->d_class_list[c], L->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lf, s->d_Lf2) ||
          pa_k_bj_pairs(s->d_class_list[c], L->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lb, s->d_Lb2))
        return 1;
  return 0;
}

static int bj_make_g4(pa_bj_t* s, int band_bits) {
  const long long tot2 = s->lay.tot2;
  const size_t esz = band_bits == 32 ? sizeof(float) : sizeof(double);
  const size_t g4_alloc = (size_t)tot2 * esz + 8192;
  s->g4_bits = band_bits;
  s->d_Lg4 = pa_rt_malloc(g4_alloc);
  if (!s->d_Lg4 || pa_rt_memset(s->d_Lg4, 0, g4_alloc))
    return BJ_FAIL("allocating the one-copy sweep records failed: %s", pa_rt_error());
  if (pa_bj_launch_g4(s)) return BJ_FAIL("k_bj_g4_setup failed");
  s->g4_bytes = (double)esz * (double)tot2;
  return 0;
}

static int bj_make_pairs(pa_bj_t* s) {
  const long long tot2 = s->lay.tot2;
  s->d_Lf2 = (double*)pa_rt_malloc(((size_t)tot2 + 1024) * sizeof(double));
  s->d_Lb2 = (double*)pa_rt_malloc(((size_t)tot2 + 1024) * sizeof(double));
  if (!s->d_Lf2 || !s->d_Lb2 ||
      pa_rt_memset(s->d_Lf2 + tot2, 0, 512 * sizeof(double)) || pa_rt_memset(s->d_Lb2 + tot2, 0, 512 * sizeof(double)))
    return BJ_FAIL("allocating the paired sweep records failed: %s", pa_rt_error());
  if (pa_bj_launch_pairs(s)) return BJ_FAIL("k_bj_pairs failed");
  s->pairs_bytes = 2.0 * 8.0 * (double)tot2;
  return 0;
}

/* Second layouts of the narrow classes for panels of up to 4 columns, made on the device from the
 * plain forward records:
 *  - bj_g4.hip (default, PREALPS_BJ_G4=0 turns it off): ONE copy for both sweeps in selective-
 *    inversion form by groups of four pivots, for classes whose blocks have at most
 *    pa_bj_g4_max_rows() rows and bands up to pa_bj_g4_max_band();
 *  - k_bj_pairs (classes R = 2, 3 that bj_g4 does not take; PREALPS_BJ_PAIRS=0 turns it off): both
 *    sweeps' records in pairs of steps for k_bj_apply_pairs.
 * Same size per block either way: 8 ceil(b / 8) (w + 4) doubles per copy.  The plain records stay for
 * the 8- and 16-column kernels.  Which class gets which, and where: the layout (class_g4, class_pairs, off2). */
static int bj_second_layouts(pa_bj_t* s, int band_bits) {
  const pa_bj_layout_t* L = &s->lay;
  const size_t np1 = (size_t)s->np + 1;
  int rc = 0;
  if (!L->any_g4 && !L->any_pairs) return 0;
  s->d_off2 = (long long*)pa_rt_malloc(np1 * sizeof(long long));
  if (!s->d_off2 || pa_rt_h2d(s->d_off2, L->off2, np1 * sizeof(long long)))
    rc = BJ_FAIL("allocating the second sweep records failed: %s", pa_rt_error());
  if (!rc && L->any_g4) rc = bj_make_g4(s, band_bits);
  if (!rc && L->any_pairs) rc = bj_make_pairs(s);
  if (!rc && pa_rt_sync()) rc = BJ_FAIL("%s", pa_rt_error());
  return rc;
}

/* ---- stage 9: the plan the kernels read, from the arrays pa_bj_t owns ------- */
static void bj_fill_plan(pa_bj_t* s) {
  pa_bj_plan_t* pl = &s->plan;
  const pa_bj_layout_t* L = &s->lay;
  /* the apply kernels take off[p] / off2[p] as the base of a block's records only: they get the READ offsets (a
   * block that repeats an earlier one reads that one's records, bj_share.h); invd, the maps and row0 stay per block */
  pl->nparts = s->np; pl->row0 = s->d_row0; pl->nrows = s->d_nrows; pl->bw = s->d_bw; pl->off = s->d_off_read;
  pl->map_f = s->d_map_f; pl->map_b = s->d_map_b; pl->Lf = s->d_Lf; pl->Lb = s->d_Lb;
  pl->invd_f = s->d_invd_f; pl->invd_b = s->d_invd_b;
  pl->Lf2 = s->d_Lf2; pl->Lb2 = s->d_Lb2; pl->off2 = s->d_off2_read;
  pl->Lg4 = s->d_Lg4; pl->g4_bits = s->d_Lg4 ? s->g4_bits : 0; pl->class_g4 = L->class_g4; pl->class_bmax = L->class_bmax;
  pl->nclass = L->nclass; pl->class_R = L->class_R; pl->class_count = L->class_count;
  pl->class_wmax = L->class_wmax;
  pl->class_list = s->class_list_c;
  pl->class_ptask = s->class_ptask; pl->pair_mode = s->pair_mode; pl->pair_intact = s->shared_blocks == s->share_members;
}

/* ---- stage 10: what a later preAlps_BlockJacobiUpdateValues needs (host memory only) ---- */
static void* bj_dup(const void* p, size_t bytes) {
  void* c = malloc(bytes ? bytes : 1);
  if (c) memcpy(c, p, bytes);
  return c;
}

static int bj_keep_decisions(pa_bj_t* s, const pa_bj_build_t* B, const pa_bj_build_in_t* in) {
  const size_t np = (size_t)B->np;
  s->h_row0 = (int*)bj_dup(B->row0, np * sizeof(int));
  s->h_nrows = (int*)bj_dup(B->nrows, np * sizeof(int));
  s->h_bw = (int*)bj_dup(B->bw, np * sizeof(int));
  s->h_is_nd = (char*)bj_dup(B->is_nd, np);
  s->h_map_f = (int*)bj_dup(B->map_f, (size_t)B->m * sizeof(int));
  s->h_grow0 = (int*)bj_dup(in->grow, np * sizeof(int));
  if (!s->h_row0 || !s->h_nrows || !s->h_bw || !s->h_is_nd || !s->h_map_f || !s->h_grow0)
    return BJ_FAIL("out of host memory for the block arrays");
  s->A_rowptr = in->rowPtr; s->op_build = pa_operator_build_count();
  return 0;
}

int preAlps_BlockJacobiCreate(CPLM_Mat_CSR_t* A, int* rowPos, int sizeRowPos, int* colPos,
                              int sizeColPos) {
  (void)colPos; (void)sizeColPos;
  PA_REQUIRE_GPU();
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built before the preconditioner");
  if (!A || !A->rowPtr || !rowPos || sizeRowPos != op->nparts + 1)
    return PA_FAIL(" wrong test 'A != NULL && sizeRowPos == nparts + 1'");
  bj_switches_t sw;
  if (bj_read_switches(&sw)) return 1;
  if (g_bj.created) preAlps_BlockJacobiFree();
  pa_bj_t* s = &g_bj;
  const pa_bj_build_in_t in = {.np = op->part1 - op->part0, .m = op->m, .rowPtr = A->rowPtr, .colInd = A->colInd, .val = A->val,
                               .grow = rowPos + op->part0, .row_off = op->row_off, .nd_mode = sw.nd_mode, .nd_rows = sw.nd_rows,
                               .dev_factor = sw.dev_factor, .dev_wmax = pa_bj_factor_wmax(), .threads = pa_host_threads()};
  s->np = in.np; s->m = in.m;
  s->row_off = in.row_off; s->dev_factor = in.dev_factor; s->dev_wmax = in.dev_wmax; s->nd_bits = sw.nd_bits;

  double t_setup0 = pa_wtime();
  /* pass 1 (parallel over blocks): RCM order, bandwidth, band assembly, host band Cholesky */
  pa_bj_build_t B;
  int rc = pa_bj_build_blocks(&in, &B);
  g_bj_setup_s[0] = pa_wtime() - t_setup0;
  t_setup0 = pa_wtime();
  if (rc == PA_BJ_NOT_SPD) rc = BJ_FAIL("diagonal block is not SPD (global row %d)", B.fail_row);
  else if (rc && B.nomem_block >= 0) rc = BJ_FAIL("out of host memory for block %d", B.nomem_block);
  else if (rc) rc = BJ_FAIL("out of host memory for the block arrays");
  /* pass 2: the layout, then the sweep layouts in this order (device allocations, uploads and syncs follow it) */
  if (!rc) {
    const pa_bj_layout_in_t lin = {.np = in.np, .nrows = B.nrows, .bw = B.bw, .is_nd = B.is_nd, .factor_wmax = in.dev_wmax,
                                   .max_R = pa_bj_max_R(), .g4_max_band = pa_bj_g4_max_band(), .g4_max_rows = pa_bj_g4_max_rows(),
                                   .dev_factor = in.dev_factor, .wide_from = sw.wide_from,
                                   .want_g4 = sw.want_g4 && (long long)in.m * 16 < 2147483647LL, .want_pairs = sw.want_pairs};
    char err[256];
    const int lrc = pa_bj_layout_build(&lin, &s->lay, err, sizeof(err));
    if (lrc == PA_BJ_BANDWIDTH) rc = BJ_FAIL("%s", err);
    else if (lrc) rc = BJ_FAIL("out of host memory for the layout of %d blocks", in.np);
  }
  if (!rc) rc = bj_share_pass(s, &B, sw.share);
  if (!rc) rc = bj_alloc_records(s);
  if (!rc) rc = bj_layout_host(s, &B);
  if (!rc) rc = bj_upload_classes(s);
  if (!rc) rc = bj_upload_index(s, &B);
  if (!rc && s->lay.ndev > 0) rc = bj_factor_device(s, &B);
  if (!rc && s->lay.nnd > 0)
    rc = pa_bj_nd_handoff("preAlps_BlockJacobiCreate", A, in.np, B.is_nd, s->lay.nnd, B.row0, B.nrows, in.grow, in.m, sw.nd_bits,
                          in.row_off);
  if (!rc) rc = bj_second_layouts(s, sw.band_bits);
  if (!rc) rc = bj_upload_share(s);
  if (!rc) rc = bj_keep_decisions(s, &B, &in);
  if (!rc) rc = bj_pair_pass(s, sw.pair);
  pa_bj_build_free(&B);
  if (rc) { preAlps_BlockJacobiFree(); return rc; }
  s->factor_bytes = 2.0 * 8.0 * (double)s->lay.tot + pa_nd_factor_bytes();
  s->nd_blocks = s->lay.nnd;
  bj_fill_plan(s);
  s->created = 1;
  ++g_bj_apply_epoch;
  pa_bj_values_epoch_sync();
  g_bj_setup_s[1] = pa_wtime() - t_setup0;
  return 0;
}

/* B_out = M^-1 A_in on the A_in->info.n current columns; the output
 * descriptor takes the input's shape (cplm_kernels.c:819-828). */
int preAlps_BlockJacobiApply(CPLM_Mat_Dense_t* A_in, CPLM_Mat_Dense_t* B_out) {
  pa_bj_t* s = &g_bj;
  if (!s->created) return PA_FAIL("preconditioner not created");
  if (!A_in || !B_out || !A_in->val || !B_out->val) return PA_FAIL(" wrong test 'A_in->val != NULL && B_out->val != NULL'");
  int ts = pa_desc_stride(A_in);
  if (pa_desc_stride(B_out) != ts || A_in->info.m != s->m)
    return PA_FAIL("panel shapes do not match the preconditioner (m %d vs %d)", A_in->info.m, s->m);
  B_out->info.n = A_in->info.n; B_out->info.N = A_in->info.N;
  B_out->info.nval = B_out->info.m * B_out->info.n;
  pa_time_begin(PA_T_PRECOND);
  /* with a coarse space the block solve must not leave its Gram by-product behind (out changes after it): an armed
   * request ends here, also one of a solver initialised before the coarse space was attached, and
   * pa_k_bj_gram_take then returns 0 */
  if (s->co.on) pa_k_bj_gram_disarm(NULL);
  if (pa_k_bj_apply(&s->plan, ts, A_in->val, B_out->val)) return PA_FAIL("block-Jacobi kernel launch failed: %s", pa_rt_error());
  if (s->nd_blocks > 0 && pa_nd_apply(ts, A_in->val, B_out->val)) return 1;
  if (s->co.on && A_in->info.n > 0) {
    if (pa_k_coarse_apply(&s->co.plan, ts, A_in->info.n, A_in->val, B_out->val)) return PA_FAIL("coarse correction failed: %s", pa_rt_error());
    ++s->co.applies;
  }
  pa_time_end(PA_T_PRECOND);
  return 0;
}

/* ---- generic handle (preAlps_preconditioner.c:20-76) ---------------------- */
int preAlps_PreconditionerCreate(PreAlps_preconditioner_t** precond, Prec_Type_t precond_type, void* data) {
  if (!precond) return PA_FAIL(" wrong test 'precond != NULL'");
  *precond = (PreAlps_preconditioner_t*)malloc(sizeof(PreAlps_preconditioner_t));
  if (!*precond) return PA_FAIL("Malloc fails for precond[].");
  (*precond)->side = LEFT_PREC;
  (*precond)->type = precond_type;
  (*precond)->data = data;
  return 0;
}

int preAlps_PreconditionerDestroy(PreAlps_preconditioner_t** precond) {
  if (precond && *precond) { free(*precond); *precond = NULL; }
  return 0;
}

int preAlps_PreconditionerMatApply(PreAlps_preconditioner_t* precond, CPLM_Mat_Dense_t* A_in,
                                   CPLM_Mat_Dense_t* B_out) {
  if (!precond) return PA_FAIL(" wrong test 'precond != NULL'");
  if (precond->type == PREALPS_BLOCKJACOBI) return preAlps_BlockJacobiApply(A_in, B_out);
  if (precond->type == PREALPS_NOPREC) {   /* CPLM_MatDenseCopy: B_out takes A_in's shape and values */
    if (!A_in || !B_out || !A_in->val || !B_out->val) return PA_FAIL(" wrong test 'A_in->val != NULL && B_out->val != NULL'");
    int ts = pa_desc_stride(A_in);
    if (pa_desc_stride(B_out) != ts || A_in->info.m != B_out->info.m)
      return PA_FAIL("panel shapes do not match (m %d vs %d)", A_in->info.m, B_out->info.m);
    B_out->info.n = A_in->info.n; B_out->info.N = A_in->info.N;
    B_out->info.nval = B_out->info.m * B_out->info.n;
    if (pa_rt_d2d(B_out->val, A_in->val, (size_t)A_in->info.m * ts * sizeof(double))) return PA_FAIL("%s", pa_rt_error());
    return 0;
  }
  return PA_FAIL("Unknown preconditioner: %d (LORASC / PRESC are not part of this library)", (int)precond->type);
}
