/*
 * bj_build.c -- the host work of creating the band block-Jacobi preconditioner (bj_build.h): every block is
 * reordered by reverse Cuthill-McKee (or left in the given order where that is no wider), assembled as a dense
 * band in factor order and, unless the device does it, factored by a band Cholesky L L^T (exact: no fill leaves
 * the band) and laid out as sweep records; the layout table says where every block's records, bands and second
 * records lie and which kernel class serves it.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_build.h"

/* ---- reverse Cuthill-McKee of one block ---------------------------------- */
typedef struct { int* xadj; int* adj; int* deg; int* order; int* pos; int* queue; int* level; } rcm_ws_t;

static int bfs_levels(int b, const int* xadj, const int* adj, int root, int* level, int* queue,
                      int stamp_unvisited, int* last_out) {
  /* level[] must hold stamp_unvisited for nodes of this component not yet seen */
  int head = 0, tail = 0, maxl = 0;
  (void)b;
  queue[tail++] = root; level[root] = 0;
  while (head < tail) {
    int u = queue[head++];
    for (int k = xadj[u]; k < xadj[u + 1]; ++k) {
      int v = adj[k];
      if (level[v] == stamp_unvisited) { level[v] = level[u] + 1; if (level[v] > maxl) maxl = level[v]; queue[tail++] = v; }
    }
  }
  *last_out = tail; /* nodes reached */
  return maxl;
}

static void rcm_order(int b, const int* xadj, const int* adj, const int* deg, int* order, int* pos,
                      int* queue, int* level) {
  const int UNSEEN = -1, DONE = -2;
  int placed = 0;
  for (int i = 0; i < b; ++i) pos[i] = UNSEEN; /* pos doubles as "placed" marker */
  while (placed < b) {
    /* seed: unplaced node of minimum degree */
    int seed = -1;
    for (int i = 0; i < b; ++i) if (pos[i] == UNSEEN && (seed < 0 || deg[i] < deg[seed])) seed = i;
    /* pseudo-peripheral root: repeat BFS from the min-degree node of the last level */
    int root = seed, ecc = -1;
    for (int it = 0; it < 6; ++it) {
      for (int i = 0; i < b; ++i) level[i] = (pos[i] == UNSEEN) ? UNSEEN : DONE;
      int reached = 0;
      int e = bfs_levels(b, xadj, adj, root, level, queue, UNSEEN, &reached);
      if (e <= ecc) break;
      ecc = e;
      int cand = -1;
      for (int q = 0; q < reached; ++q) { int u = queue[q]; if (level[u] == e && (cand < 0 || deg[u] < deg[cand])) cand = u; }
      if (cand < 0 || cand == root) break;
      root = cand;
    }
    /* Cuthill-McKee from root, neighbours by increasing degree */
    int head = placed, tail = placed;
    order[tail++] = root; pos[root] = DONE;
    while (head < tail) {
      int u = order[head++];
      int s0 = tail;
      for (int k = xadj[u]; k < xadj[u + 1]; ++k) { int v = adj[k]; if (pos[v] == UNSEEN) { pos[v] = DONE; order[tail++] = v; } }
      for (int a = s0 + 1; a < tail; ++a) { /* insertion sort by degree */
        int v = order[a], c = a;
        while (c > s0 && deg[order[c - 1]] > deg[v]) { order[c] = order[c - 1]; --c; }
        order[c] = v;
      }
    }
    placed = tail;
  }
  for (int i = 0; i < b / 2; ++i) { int t = order[i]; order[i] = order[b - 1 - i]; order[b - 1 - i] = t; }
  for (int i = 0; i < b; ++i) pos[order[i]] = i;
}

/* ---- per-block host work ------------------------------------------------- */
static void bj_block_graph_free(rcm_ws_t* g) {
  free(g->xadj); free(g->adj); free(g->deg); free(g->order); free(g->pos); free(g->queue); free(g->level);
  memset(g, 0, sizeof(*g));
}

/* Adjacency of block q's rows among themselves (no diagonal) + the work arrays of rcm_order.  Non-zero and
 * nothing allocated: out of memory. */
static int bj_block_graph(const pa_bj_build_in_t* in, const pa_bj_build_t* B, int q, rcm_ws_t* g) {
  const int r0 = B->row0[q], b = B->nrows[q];
  const int g0 = in->grow[q], g1 = g0 + b;
  int nadj = 0;
  for (int i = 0; i < b; ++i)
    for (int k = in->rowPtr[r0 + i]; k < in->rowPtr[r0 + i + 1]; ++k) { int c = in->colInd[k]; if (c >= g0 && c < g1 && c != g0 + i) ++nadj; }
  g->xadj = (int*)malloc(((size_t)b + 1) * sizeof(int));
  g->adj = (int*)malloc((size_t)(nadj ? nadj : 1) * sizeof(int));
  g->deg = (int*)malloc((size_t)(b ? b : 1) * sizeof(int));
  g->order = (int*)malloc((size_t)(b ? b : 1) * sizeof(int));
  g->pos = (int*)malloc((size_t)(b ? b : 1) * sizeof(int));
  g->queue = (int*)malloc((size_t)(b ? b : 1) * sizeof(int));
  g->level = (int*)malloc((size_t)(b ? b : 1) * sizeof(int));
  if (!g->xadj || !g->adj || !g->deg || !g->order || !g->pos || !g->queue || !g->level) { bj_block_graph_free(g); return 1; }
  g->xadj[0] = 0;
  for (int i = 0; i < b; ++i) {
    int e = g->xadj[i];
    for (int k = in->rowPtr[r0 + i]; k < in->rowPtr[r0 + i + 1]; ++k) { int c = in->colInd[k]; if (c >= g0 && c < g1 && c != g0 + i) g->adj[e++] = c - g0; }
    g->xadj[i + 1] = e; g->deg[i] = e - g->xadj[i];
  }
  return 0;
}

/* Factor order of the block (g->order / g->pos) and its bandwidth.  RCM is a heuristic: on elongated boxes
 * of a structured grid the given row order (long axis slowest) can have the narrower band -- keep whichever
 * is narrower. */
static int bj_block_order(int b, rcm_ws_t* g) {
  rcm_order(b, g->xadj, g->adj, g->deg, g->order, g->pos, g->queue, g->level);
  int w = 0, wnat = 0;
  for (int i = 0; i < b; ++i)
    for (int k = g->xadj[i]; k < g->xadj[i + 1]; ++k) {
      int dd = g->pos[i] - g->pos[g->adj[k]]; if (dd < 0) dd = -dd; if (dd > w) w = dd;
      int dn = i - g->adj[k]; if (dn < 0) dn = -dn; if (dn > wnat) wnat = dn;
    }
  if (wnat <= w) { w = wnat; for (int i = 0; i < b; ++i) { g->order[i] = i; g->pos[i] = i; } }
  return w;
}

/* Row-major band of block q in factor order: band[i*(w+1) + d] = A(new i, new i-d).  NULL: out of memory. */
static double* bj_band_rows(const pa_bj_build_in_t* in, const pa_bj_build_t* B, int q, const int* pos, int w) {
  const int r0 = B->row0[q], b = B->nrows[q];
  const int g0 = in->grow[q], g1 = g0 + b;
  const size_t len = (size_t)b * (w + 1);
  double* band = (double*)calloc(len ? len : 1, sizeof(double));
  if (!band) return NULL;
  for (int i = 0; i < b; ++i) {
    int ni = pos[i];
    for (int k = in->rowPtr[r0 + i]; k < in->rowPtr[r0 + i + 1]; ++k) {
      int c = in->colInd[k];
      if (c < g0 || c >= g1) continue;
      int nj = pos[c - g0];
      if (nj <= ni) band[(size_t)ni * (w + 1) + (ni - nj)] = in->val[k];
    }
  }
  return band;
}

/* Blocks that go to the blocked device factorisation (k_bj_factor_big) are assembled diagonal-major
 * instead, band[d*b + i], and only the entries travel: (offset in the block's band, value).  Non-zero and
 * nothing kept: out of memory. */
static int bj_band_coo(const pa_bj_build_in_t* in, pa_bj_build_t* B, int q, const int* pos) {
  const int r0 = B->row0[q], b = B->nrows[q];
  const int g0 = in->grow[q], g1 = g0 + b;
  size_t cnt = 0;
  for (int i = 0; i < b; ++i)
    for (int k = in->rowPtr[r0 + i]; k < in->rowPtr[r0 + i + 1]; ++k) {
      int c = in->colInd[k];
      if (c >= g0 && c < g1 && pos[c - g0] <= pos[i]) ++cnt;
    }
  long long* co = (long long*)malloc((cnt ? cnt : 1) * sizeof(long long));
  double* cv = (double*)malloc((cnt ? cnt : 1) * sizeof(double));
  if (!co || !cv) { free(co); free(cv); return 1; }
  cnt = 0;
  for (int i = 0; i < b; ++i) {
    int ni = pos[i];
    for (int k = in->rowPtr[r0 + i]; k < in->rowPtr[r0 + i + 1]; ++k) {
      int c = in->colInd[k];
      if (c < g0 || c >= g1) continue;
      int nj = pos[c - g0];
      if (nj > ni) continue;
      co[cnt] = (long long)(ni - nj) * b + ni; cv[cnt] = in->val[k]; ++cnt;
    }
  }
  B->coo_off[q] = co; B->coo_val[q] = cv; B->coo_n[q] = cnt;
  return 0;
}

int pa_bj_band_cholesky(double* band, int b, int w) {
  const size_t ld = (size_t)w + 1;
  int bad = -1;
  for (int i = 0; i < b; ++i) {
    double* Li = band + (size_t)i * ld; /* Li[d] = L(i, i-d) */
    int jlo = i - w > 0 ? i - w : 0;
    for (int j = jlo; j < i; ++j) {
      const double* Lj = band + (size_t)j * ld;
      int klo = j - w > jlo ? j - w : jlo;
      double sum = Li[i - j];
      for (int k = klo; k < j; ++k) sum -= Li[i - k] * Lj[j - k];
      Li[i - j] = sum / Lj[0];
    }
    double dsum = Li[0];
    for (int k = jlo; k < i; ++k) dsum -= Li[i - k] * Li[i - k];
    if (!(dsum > 0.0)) { if (bad < 0) bad = i; dsum = NAN; }
    Li[0] = sqrt(dsum);
  }
  return bad;
}

static void bj_block_nomem(pa_bj_build_t* B, int q, int* nomem) {
#pragma omp critical
  { if (!*nomem) { *nomem = 1; B->nomem_block = q; } }
}

/* One block: order, bandwidth, the sparse-factor decision, band assembly, host band Cholesky.  The device
 * factors every band (k_bj_factor / k_bj_factor_big) unless !dev_factor. */
static void bj_host_block(const pa_bj_build_in_t* in, pa_bj_build_t* B, int q, int* nomem) {
  const int r0 = B->row0[q], b = B->nrows[q];
  rcm_ws_t g;
  if (bj_block_graph(in, B, q, &g)) { bj_block_nomem(B, q, nomem); return; }
  const int w = B->bw[q] = bj_block_order(b, &g);
  if (in->nd_mode && b >= in->nd_rows && (in->nd_mode >= 2 || w > 256)) {
    B->is_nd[q] = 1;
    for (int j = 0; j < b; ++j) { B->map_f[r0 + j] = j; B->map_b[r0 + j] = b - 1 - j; }
    bj_block_graph_free(&g);
    return;
  }
  int bad_alloc;
  if (in->dev_factor && w > in->dev_wmax) bad_alloc = bj_band_coo(in, B, q, g.pos);
  else bad_alloc = !(B->bands[q] = bj_band_rows(in, B, q, g.pos, w));
  if (bad_alloc) { bj_block_nomem(B, q, nomem); bj_block_graph_free(&g); return; }
  if (!in->dev_factor) {
    const int bad = pa_bj_band_cholesky(B->bands[q], b, w);
    if (bad >= 0) {
#pragma omp critical
      { if (B->fail_row < 0) B->fail_row = in->row_off + r0 + g.order[bad]; }
    }
  }
  for (int j = 0; j < b; ++j) {
    B->map_f[r0 + j] = g.order[j];
    B->map_b[r0 + j] = g.order[b - 1 - j];
  }
  bj_block_graph_free(&g);
}

void pa_bj_build_free(pa_bj_build_t* B) {
  for (int q = 0; q < B->np; ++q) {
    if (B->bands) free(B->bands[q]);
    if (B->coo_off) free(B->coo_off[q]);
    if (B->coo_val) free(B->coo_val[q]);
  }
  free(B->bands); free(B->coo_off); free(B->coo_val); free(B->coo_n);
  free(B->row0); free(B->nrows); free(B->bw); free(B->is_nd); free(B->map_f); free(B->map_b);
  free(B->invd_f); free(B->invd_b);
  memset(B, 0, sizeof(*B));
  B->fail_row = B->nomem_block = -1;
}

int pa_bj_build_blocks(const pa_bj_build_in_t* in, pa_bj_build_t* B) {
  const int np = in->np, m = in->m;
  const size_t np1 = (size_t)(np ? np : 1), m1 = (size_t)(m ? m : 1);
  memset(B, 0, sizeof(*B));
  B->np = np; B->m = m;
  B->fail_row = B->nomem_block = -1;
  B->row0 = (int*)malloc(np1 * sizeof(int));
  B->nrows = (int*)malloc(np1 * sizeof(int));
  B->bw = (int*)calloc(np1, sizeof(int));
  B->is_nd = (char*)calloc(np1, 1);
  B->map_f = (int*)malloc(m1 * sizeof(int));
  B->map_b = (int*)malloc(m1 * sizeof(int));
  B->invd_f = (double*)malloc(m1 * sizeof(double));
  B->invd_b = (double*)malloc(m1 * sizeof(double));
  B->bands = (double**)calloc(np1, sizeof(double*));
  B->coo_off = (long long**)calloc(np1, sizeof(long long*));
  B->coo_val = (double**)calloc(np1, sizeof(double*));
  B->coo_n = (size_t*)calloc(np1, sizeof(size_t));
  if (!B->row0 || !B->nrows || !B->bw || !B->is_nd || !B->map_f || !B->map_b || !B->invd_f || !B->invd_b ||
      !B->bands || !B->coo_off || !B->coo_val || !B->coo_n) {
    pa_bj_build_free(B);
    return PA_BJ_NOMEM;
  }
  for (int q = 0; q < np; ++q) {
    B->row0[q] = in->grow[q] - in->row_off;
    B->nrows[q] = in->grow[q + 1] - in->grow[q];
  }
  int nomem = 0;
#pragma omp parallel for num_threads(in->threads > 0 ? in->threads : 1) schedule(dynamic, 1)
  for (int q = 0; q < np; ++q) bj_host_block(in, B, q, &nomem);
  if (nomem || B->fail_row >= 0) {
    const int fail_row = B->fail_row, nomem_block = B->nomem_block;
    pa_bj_build_free(B);
    if (nomem) { B->nomem_block = nomem_block; return PA_BJ_NOMEM; }
    B->fail_row = fail_row;
    return PA_BJ_NOT_SPD;
  }
  return PA_BJ_OK;
}

void pa_bj_layout_slab(pa_bj_build_t* B, int wide_from, int x, int j0, double* f, double* g) {
  const int b = B->nrows[x], w = B->bw[x], r0 = B->row0[x];
  const size_t ld = (size_t)w + 1;
  const int wide = w > wide_from;
  const size_t reclen = (size_t)pa_bj_reclen(w, wide_from);
  const double* band = B->bands[x];
  double* invd_f = B->invd_f; double* invd_b = B->invd_b;
  const int j1 = j0 + 256 < b ? j0 + 256 : b;
  for (int j = j0; j < j1; ++j) {
    int jr = b - 1 - j;
    invd_f[r0 + j] = 1.0 / band[(size_t)j * ld];
    invd_b[r0 + j] = 1.0 / band[(size_t)jr * ld];
    for (int dd = 1; dd <= w; ++dd) {
      if (wide) { /* window-slot order, pre-divided by the pivot */
        if (j + dd < b) f[(size_t)j * reclen + (size_t)(j + dd) % reclen] = band[(size_t)(j + dd) * ld + dd] * invd_f[r0 + j];
        if (jr - dd >= 0) g[(size_t)j * reclen + (size_t)(j + dd) % reclen] = band[(size_t)jr * ld + dd] * invd_b[r0 + j];
      } else {    /* [L(j+1..j+w, j) / L(j,j) | 0] (see bj_band.hip: bj_block) */
        f[(size_t)j * reclen + dd - 1] = (j + dd < b) ? band[(size_t)(j + dd) * ld + dd] * invd_f[r0 + j] : 0.0;
        g[(size_t)j * reclen + dd - 1] = (jr - dd >= 0) ? band[(size_t)jr * ld + dd] * invd_b[r0 + j] : 0.0;
      }
    }
  }
}

/* ---- the layout ------------------------------------------------------------ */
void pa_bj_layout_free(pa_bj_layout_t* L) {
  for (int c = 0; c < PA_BJ_MAX_CLASSES; ++c) free(L->class_list[c]);
  free(L->off); free(L->off2); free(L->boff); free(L->slist); free(L->blist);
  memset(L, 0, sizeof(*L));
}

static int layout_fail(pa_bj_layout_t* L, int rc, int bad_bw) {
  pa_bj_layout_free(L);
  L->bad_bw = bad_bw;
  return rc;
}

int pa_bj_layout_build(const pa_bj_layout_in_t* in, pa_bj_layout_t* L, char* err, size_t errlen) {
  const int np = in->np;
  const size_t np1 = (size_t)np + 1;
  memset(L, 0, sizeof(*L));
  if (err && errlen) err[0] = 0;
  L->np = np;
  /* Bands above wide_from get one workgroup per block (k_bj_wide) instead of one wavefront: always above
   * 64 * max_R - 64, where the wavefront's registers end, and from factor_wmax + 1 on when the blocks are too few
   * to give every SIMD a wavefront.  The device factorisation lays out window-slot records only for bands above
   * factor_wmax. */
  const int wf_lo = in->factor_wmax, wf_hi = 64 * in->max_R - 64;
  L->wide_from = np < 1024 ? wf_lo : wf_hi;
  if (in->wide_from >= 0) {
    L->wide_from = in->wide_from;
    if (L->wide_from < wf_lo) L->wide_from = wf_lo;
    if (L->wide_from > wf_hi) L->wide_from = wf_hi;
  }
  L->off = (long long*)calloc(np1, sizeof(long long));
  L->off2 = (long long*)calloc(np1, sizeof(long long));
  L->boff = (long long*)calloc(np1, sizeof(long long));
  L->slist = (int*)malloc(np1 * sizeof(int));
  L->blist = (int*)malloc(np1 * sizeof(int));
  int* cls = (int*)malloc(np1 * sizeof(int));
  if (!L->off || !L->off2 || !L->boff || !L->slist || !L->blist || !cls) { free(cls); return layout_fail(L, PA_BJ_NOMEM, 0); }
  /* records, bands, launch lists, classes: one pass over the blocks */
  int maxw = 0;
  long long btot = 0;
  for (int q = 0; q < np; ++q) {
    const int w = in->bw[q], b = in->nrows[q];
    const long long reclen = pa_bj_reclen(w, L->wide_from);
    cls[q] = -1;
    L->boff[q] = btot;
    if (w > L->max_bw) L->max_bw = w;
    if (in->is_nd[q]) { L->off[q + 1] = L->off[q]; ++L->nnd; continue; }     /* no band records: sparse factor */
    if (w <= L->wide_from && reclen > L->maxrec) L->maxrec = reclen;
    if (in->dev_factor) ++L->ndev;
    L->off[q + 1] = L->off[q] + (long long)b * reclen;
    if (w > maxw) maxw = w;
    btot += pa_bj_band_len(b, w, 0);
    if (w <= in->factor_wmax) { L->slist[L->ns++] = q; if (w > L->wsmall) L->wsmall = w; }
    else { L->blist[L->nbig++] = q; if (w > L->wbig) L->wbig = w; }
    int R = (w + 127) / 64, c;
    if (w > L->wide_from) { /* wide classes: -(register sets per lane) */
      const int W = pa_bj_wide_window(w);
      R = W <= 1024 ? -1 : (W <= 2048 ? -2 : -4);
    }
    for (c = 0; c < L->nclass; ++c) if (L->class_R[c] == R) break;
    if (c == L->nclass) { L->class_R[c] = R; L->nclass++; }     /* (count, wmax, bmax: zero from the memset) */
    cls[q] = c; L->class_count[c]++;
    if (w > L->class_wmax[c]) L->class_wmax[c] = w;
    if (b > L->class_bmax[c]) L->class_bmax[c] = b;
  }
  L->boff[np] = btot; L->btot = (size_t)btot;
  if (pa_bj_wide_window(maxw) > 4096) {
    free(cls);
    if (err) snprintf(err, errlen, "block-Jacobi: a diagonal block has bandwidth %d after reordering; the workgroup-resident "
                      "solve supports up to 4032 -- use more (smaller) subdomains", maxw);
    return layout_fail(L, PA_BJ_BANDWIDTH, maxw);
  }
  L->tot = (size_t)L->off[np];
  /* A narrow block is streamed in chunks of 8 steps, whole KiB each: the last chunk of a block whose rows are no
   * multiple of 8 reads up to 7 records and 1 KiB beyond the block -- behind the last block, into this slack. */
  L->pad = 256 + 8 * (size_t)L->maxrec;
  for (int c = 0; c < L->nclass; ++c) {
    int n = 0;
    L->class_list[c] = (int*)malloc((size_t)L->class_count[c] * sizeof(int));
    if (!L->class_list[c]) { free(cls); return layout_fail(L, PA_BJ_NOMEM, 0); }
    for (int q = 0; q < np; ++q) if (cls[q] == c) L->class_list[c][n++] = q;
  }
  free(cls);
  /* Second layouts of the narrow classes for panels of up to 4 columns: the one-copy records of bj_g4.hip for
   * classes whose blocks have at most g4_max_rows rows and bands up to g4_max_band, the paired records of
   * k_bj_pairs for the classes R = 2, 3 that bj_g4 does not take.  Same size per block either way. */
  for (int c = 0; c < L->nclass; ++c) {
    L->class_g4[c] = in->want_g4 && L->class_R[c] > 0 && L->class_wmax[c] <= in->g4_max_band && L->class_bmax[c] <= in->g4_max_rows;
    L->class_pairs[c] = in->want_pairs && !L->class_g4[c] && (L->class_R[c] == 2 || L->class_R[c] == 3);
    L->any_g4 |= L->class_g4[c]; L->any_pairs |= L->class_pairs[c];
  }
  if (L->any_g4 || L->any_pairs)
    for (int q = 0; q < np; ++q) {
      if (in->is_nd[q] || in->bw[q] > L->wide_from) continue;
      L->off2[q] = L->tot2;                                 /* (blocks of the other classes: unused) */
      L->tot2 += 8LL * ((in->nrows[q] + 7) / 8) * (in->bw[q] + 4);
    }
  return PA_BJ_OK;
}
