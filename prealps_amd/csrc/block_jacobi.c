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
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pa_host.h"
#include "bj_band_map.h"
#include "coarse_space.h"

/* The coarse space attached to the preconditioner (preAlps_BlockJacobiSetCoarseSpace): what the caller gave, kept on
 * the host for preAlps_BlockJacobiUpdateValues, and the device arrays pa_k_coarse_apply reads. */
typedef struct {
  int on;
  int k, naggr, nc, nchunks, n;
  double* V;                  /* the caller's vectors, n x k column major, in the caller's order and units */
  int* part_aggregate;        /* np */
  double* d_zv; int* d_ch_row0; int* d_ch_nrows; int* d_ch_aggr; int* d_agg_ptr; int* d_agg_chunk;
  double* d_Einv; double* d_partial; double* d_c; double* d_y;
  pa_coarse_plan_t plan;
  double bytes, setup_s;
  int builds; long long applies;
} pa_bj_coarse_t;

typedef struct {
  int created;
  pa_bj_coarse_t co;
  int np;                 /* local blocks */
  int m;
  /* device */
  int* d_row0; int* d_nrows; int* d_bw; long long* d_off;
  int* d_map_f; int* d_map_b;
  double* d_Lf; double* d_Lb; double* d_invd_f; double* d_invd_b;
  double* d_Lf2; double* d_Lb2; long long* d_off2;     /* paired records of the narrow classes (optional) */
  double pairs_bytes;
  void* d_Lg4; int g4_bits; double g4_bytes;                   /* one-copy records of bj_g4.hip (optional) */
  int class_g4[16]; int class_bmax[16];
  /* classes by register sets */
  int nclass; int class_R[16]; int class_count[16]; int class_wmax[16]; int* class_list[16];
  const int* class_list_c[16];
  pa_bj_plan_t plan;
  double factor_bytes; int max_bw; int nd_blocks;
  /* What preAlps_BlockJacobiUpdateValues needs of the create, so that it reads no switch again and repeats no
   * decision: the host copies of the per-block arrays and of the factor order, the switches as the create read
   * them, and what tells that operator and panel are still the create's. */
  int* h_row0; int* h_nrows; int* h_bw; int* h_grow0; int* h_map_f; char* h_is_nd;
  int row_off, wide_from, dev_factor, dev_wmax, nd_bits;
  int class_pairs[16];           /* 1: the class has paired records in Lf2 / Lb2 */
  size_t tot;                    /* doubles of the plain records, per sweep */
  const int* A_rowptr;           /* rowPtr of the create's A */
  int op_build;                  /* pa_operator_build_count() at the create */
  /* the band map on the device (bj_band_map.h) and the launch lists of the two factorisation kernels, cut at the
   * first update and kept until the preconditioner is freed */
  unsigned* d_bm_src; unsigned* d_bm_dst; int* d_bm_chunk_blk; unsigned* d_bm_chunk_first;
  size_t bm_n, bm_nchunks, bm_bytes, btot;
  long long* d_boff; int* d_slist; int* d_blist; int* d_fail;
  int ns, nbig, wsmall, wbig;
  int bm_builds, updates, nd_rebuilt;
  double upd_map_s, upd_copy_s, upd_kernel_s, upd_total_s;
} pa_bj_t;

/* block that holds local (factor-order) position `pos` */
static int part_of_local_row(const int* row0, const int* nrows, int np, int pos) {
  for (int q = 0; q < np; ++q) if (pos >= row0[q] && pos < row0[q] + nrows[q]) return q;
  return 0;
}

static pa_bj_t g_bj;
static double g_bj_setup_s[2];
double pa_bj_setup_seconds(int which) { return g_bj_setup_s[which ? 1 : 0]; }

double pa_bj_factor_bytes(void) { return g_bj.created ? g_bj.factor_bytes : 0.0; }
static int g_bj_values_epoch;   /* pa_operator_values_epoch() at the last create: a smaller one than the operator's means a lagged factor */
int pa_bj_values_epoch(void) { return g_bj_values_epoch; }
int pa_bj_max_bandwidth(void) { return g_bj.created ? g_bj.max_bw : 0; }
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
  if (!s->created || s->nd_blocks > 0 || !s->d_Lg4 || s->nclass != 1 || !s->class_g4[0] || s->class_count[0] != s->np) return 0;
  if (s->co.on) return 0;      /* the coarse correction changes `out` after the block solve: its Gram block would be stale */
  return s->np;
}

/* + 1 whenever what preAlps_BlockJacobiApply launches or the device arrays it reads change: a create, a free, a coarse
 * space set, replaced, cleared or dropped.  A solver that replays captured iteration segments (ecg.c: seg_begin)
 * compares it and captures anew: its graphs hold the old launches and the old pointers. */
static int g_bj_apply_epoch;
int pa_bj_apply_epoch(void) { return g_bj_apply_epoch; }

static void bj_coarse_release(pa_bj_coarse_t* co) {
  pa_rt_free(co->d_zv); pa_rt_free(co->d_ch_row0); pa_rt_free(co->d_ch_nrows); pa_rt_free(co->d_ch_aggr);
  pa_rt_free(co->d_agg_ptr); pa_rt_free(co->d_agg_chunk); pa_rt_free(co->d_Einv); pa_rt_free(co->d_partial);
  pa_rt_free(co->d_c); pa_rt_free(co->d_y);
  free(co->V); free(co->part_aggregate);
  memset(co, 0, sizeof(*co));
}

void preAlps_BlockJacobiFree(void) {
  pa_bj_t* s = &g_bj;
  bj_coarse_release(&s->co);
  ++g_bj_apply_epoch;
  pa_rt_free(s->d_row0); pa_rt_free(s->d_nrows); pa_rt_free(s->d_bw); pa_rt_free(s->d_off);
  pa_rt_free(s->d_map_f); pa_rt_free(s->d_map_b);
  pa_rt_free(s->d_Lf); pa_rt_free(s->d_Lb); pa_rt_free(s->d_invd_f); pa_rt_free(s->d_invd_b);
  pa_rt_free(s->d_Lf2); pa_rt_free(s->d_Lb2); pa_rt_free(s->d_off2); pa_rt_free(s->d_Lg4);
  for (int c = 0; c < 16; ++c) pa_rt_free(s->class_list[c]);
  free(s->h_row0); free(s->h_nrows); free(s->h_bw); free(s->h_grow0); free(s->h_map_f); free(s->h_is_nd);
  pa_rt_free(s->d_bm_src); pa_rt_free(s->d_bm_dst); pa_rt_free(s->d_bm_chunk_blk); pa_rt_free(s->d_bm_chunk_first);
  pa_rt_free(s->d_boff); pa_rt_free(s->d_slist); pa_rt_free(s->d_blist); pa_rt_free(s->d_fail);
  pa_nd_free();
  memset(s, 0, sizeof(*s));
}

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

/* ---- creation: one build context, one stage per step ------------------------ */
/* The stages report as the entry point they belong to: the error texts name preAlps_BlockJacobiCreate. */
#define BJ_FAIL(...) pa_fail_at("preAlps_BlockJacobiCreate", __VA_ARGS__)

/* What the host holds while the preconditioner is being created: the inputs and switches of the create, the
 * per-block and per-row arrays every stage reads, and the assembled bands on their way to the device.  One
 * owner: bj_build_release frees all of it on every way out (bands[x] already released after its upload is
 * NULL by then). */
typedef struct {
  const CPLM_Mat_CSR_t* A; const int* rowPos; const pa_operator_info_t* op;
  int np, m, row_off;
  int nd_bits, band_bits;     /* storage of the sparse factors / of the one-copy band records */
  int nd_mode, nd_rows;       /* PREALPS_BJ_ND, PREALPS_BJ_ND_ROWS */
  int dev_factor, dev_wmax;   /* PREALPS_BJ_FACTOR != host; widest band of k_bj_factor */
  int* row0; int* nrows; int* bw; char* is_nd;
  long long* off;             /* np + 1: record offsets */
  int* map_f; int* map_b; double* invd_f; double* invd_b;
  double** bands;             /* row-major bands (host-factored when !dev_factor) */
  long long** coo_off; double** coo_val; size_t* coo_n;   /* wide blocks, device path: entries only */
  int fail_row;
  int wide_from; size_t tot; int ndev, nnd;
} bj_build_t;

static void bj_build_init(bj_build_t* B, const CPLM_Mat_CSR_t* A, const int* rowPos, const pa_operator_info_t* op) {
  memset(B, 0, sizeof(*B));
  B->A = A; B->rowPos = rowPos; B->op = op;
  const int np = B->np = op->part1 - op->part0, m = B->m = op->m;
  B->row_off = op->row_off;
  B->row0 = (int*)malloc(np * sizeof(int));
  B->nrows = (int*)malloc(np * sizeof(int));
  B->bw = (int*)calloc(np, sizeof(int));
  B->off = (long long*)malloc((np + 1) * sizeof(long long));
  B->map_f = (int*)malloc((size_t)(m ? m : 1) * sizeof(int));
  B->map_b = (int*)malloc((size_t)(m ? m : 1) * sizeof(int));
  B->invd_f = (double*)malloc((size_t)(m ? m : 1) * sizeof(double));
  B->invd_b = (double*)malloc((size_t)(m ? m : 1) * sizeof(double));
  B->bands = (double**)calloc(np, sizeof(double*));
  B->coo_off = (long long**)calloc(np, sizeof(long long*));
  B->coo_val = (double**)calloc(np, sizeof(double*));
  B->coo_n = (size_t*)calloc(np, sizeof(size_t));
  B->is_nd = (char*)calloc(np ? np : 1, 1);
  B->fail_row = -1;
  for (int q = 0; q < np; ++q) {
    B->row0[q] = rowPos[op->part0 + q] - B->row_off;
    B->nrows[q] = rowPos[op->part0 + q + 1] - rowPos[op->part0 + q];
  }
  /* Large blocks (few subdomains of thousands of rows, the reference's own regime) get a sparse
   * nested-dissection factor instead of a band (nd.c).  PREALPS_BJ_ND: 0 never, 1 (default) for
   * blocks of at least PREALPS_BJ_ND_ROWS (2048) rows whose band exceeds 256, 2 for every block of
   * at least PREALPS_BJ_ND_ROWS rows.  (Measured on elasticity 70^3, per apply: blocks of 17.5 k rows
   * 2.3 ms against 15.3 ms with the band kernels; 2187 rows 1.35 against 1.46 ms; 648 rows 0.90
   * against 0.60 ms: small blocks stay with the band.) */
  B->nd_mode = getenv("PREALPS_BJ_ND") ? atoi(getenv("PREALPS_BJ_ND")) : 1;
  B->nd_rows = getenv("PREALPS_BJ_ND_ROWS") ? atoi(getenv("PREALPS_BJ_ND_ROWS")) : 2048;
  /* PREALPS_BJ_FACTOR=host keeps every factorisation on the host threads */
  const char* fenv = getenv("PREALPS_BJ_FACTOR");
  B->dev_factor = !(fenv && !strcmp(fenv, "host"));
  B->dev_wmax = pa_bj_factor_wmax();
}

static void bj_build_release(bj_build_t* B) {
  for (int q = 0; q < B->np; ++q) { free(B->bands[q]); free(B->coo_off[q]); free(B->coo_val[q]); }
  free(B->bands); free(B->coo_off); free(B->coo_val); free(B->coo_n);
  free(B->row0); free(B->nrows); free(B->bw); free(B->off); free(B->map_f); free(B->map_b);
  free(B->invd_f); free(B->invd_b); free(B->is_nd);
}

/* Storage bits of a factor: the value set through the API, else the switch `name` (double / single). */
static int bj_storage_bits(int set, const char* name, const char* what, int* bits) {
  const char* pe = getenv(name);
  if (set) *bits = set;
  else if (!pe || !*pe || !strcmp(pe, "double")) *bits = 64;
  else if (!strcmp(pe, "single")) *bits = 32;
  else return BJ_FAIL("%s=%s: expected double or single (storage of the %s)", name, pe, what);
  return 0;
}

/* ---- stage 1: per-block host work ------------------------------------------ */
/* Adjacency of block q's rows among themselves (no diagonal) + the work arrays of rcm_order. */
static void bj_block_graph(const bj_build_t* B, int q, rcm_ws_t* g) {
  const CPLM_Mat_CSR_t* A = B->A;
  const int r0 = B->row0[q], b = B->nrows[q];
  const int g0 = B->rowPos[B->op->part0 + q], g1 = g0 + b;
  int nadj = 0;
  for (int i = 0; i < b; ++i)
    for (int k = A->rowPtr[r0 + i]; k < A->rowPtr[r0 + i + 1]; ++k) { int c = A->colInd[k]; if (c >= g0 && c < g1 && c != g0 + i) ++nadj; }
  g->xadj = (int*)malloc((b + 1) * sizeof(int));
  g->adj = (int*)malloc((nadj ? nadj : 1) * sizeof(int));
  g->deg = (int*)malloc(b * sizeof(int));
  g->order = (int*)malloc(b * sizeof(int));
  g->pos = (int*)malloc(b * sizeof(int));
  g->queue = (int*)malloc(b * sizeof(int));
  g->level = (int*)malloc(b * sizeof(int));
  g->xadj[0] = 0;
  for (int i = 0; i < b; ++i) {
    int e = g->xadj[i];
    for (int k = A->rowPtr[r0 + i]; k < A->rowPtr[r0 + i + 1]; ++k) { int c = A->colInd[k]; if (c >= g0 && c < g1 && c != g0 + i) g->adj[e++] = c - g0; }
    g->xadj[i + 1] = e; g->deg[i] = e - g->xadj[i];
  }
}

static void bj_block_graph_free(rcm_ws_t* g) {
  free(g->xadj); free(g->adj); free(g->deg); free(g->order); free(g->pos); free(g->queue); free(g->level);
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

/* Row-major band of block q in factor order: band[i*(w+1) + d] = A(new i, new i-d). */
static double* bj_band_rows(const bj_build_t* B, int q, const int* pos, int w) {
  const CPLM_Mat_CSR_t* A = B->A;
  const int r0 = B->row0[q], b = B->nrows[q];
  const int g0 = B->rowPos[B->op->part0 + q], g1 = g0 + b;
  double* band = (double*)calloc((size_t)b * (w + 1), sizeof(double));
  for (int i = 0; i < b; ++i) {
    int ni = pos[i];
    for (int k = A->rowPtr[r0 + i]; k < A->rowPtr[r0 + i + 1]; ++k) {
      int c = A->colInd[k];
      if (c < g0 || c >= g1) continue;
      int nj = pos[c - g0];
      if (nj <= ni) band[(size_t)ni * (w + 1) + (ni - nj)] = A->val[k];
    }
  }
  return band;
}

/* Blocks that go to the blocked device factorisation (k_bj_factor_big) are assembled diagonal-major
 * instead, band[d*b + i], and only the entries travel: (offset in the block's band, value). */
static void bj_band_coo(bj_build_t* B, int q, const int* pos) {
  const CPLM_Mat_CSR_t* A = B->A;
  const int r0 = B->row0[q], b = B->nrows[q];
  const int g0 = B->rowPos[B->op->part0 + q], g1 = g0 + b;
  size_t cnt = 0;
  for (int i = 0; i < b; ++i)
    for (int k = A->rowPtr[r0 + i]; k < A->rowPtr[r0 + i + 1]; ++k) {
      int c = A->colInd[k];
      if (c >= g0 && c < g1 && pos[c - g0] <= pos[i]) ++cnt;
    }
  long long* co = (long long*)malloc((cnt ? cnt : 1) * sizeof(long long));
  double* cv = (double*)malloc((cnt ? cnt : 1) * sizeof(double));
  cnt = 0;
  for (int i = 0; i < b; ++i) {
    int ni = pos[i];
    for (int k = A->rowPtr[r0 + i]; k < A->rowPtr[r0 + i + 1]; ++k) {
      int c = A->colInd[k];
      if (c < g0 || c >= g1) continue;
      int nj = pos[c - g0];
      if (nj > ni) continue;
      co[cnt] = (long long)(ni - nj) * b + ni; cv[cnt] = A->val[k]; ++cnt;
    }
  }
  B->coo_off[q] = co; B->coo_val[q] = cv; B->coo_n[q] = cnt;
}

/* In-place band Cholesky on the host (band[i*(w+1) + d] = L(i, i-d)); returns the first row whose pivot is
 * not positive (the factor carries NaN from there on), -1 if none. */
static int bj_band_cholesky(double* band, int b, int w) {
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

/* One block: order, bandwidth, the sparse-factor decision, band assembly, host band Cholesky.  The device
 * factors every band (k_bj_factor / k_bj_factor_big) unless PREALPS_BJ_FACTOR=host. */
static void bj_host_block(bj_build_t* B, int q) {
  const int r0 = B->row0[q], b = B->nrows[q];
  rcm_ws_t g;
  bj_block_graph(B, q, &g);
  const int w = B->bw[q] = bj_block_order(b, &g);
  if (B->nd_mode && b >= B->nd_rows && (B->nd_mode >= 2 || w > 256)) {
    B->is_nd[q] = 1;
    for (int j = 0; j < b; ++j) { B->map_f[r0 + j] = j; B->map_b[r0 + j] = b - 1 - j; }
    bj_block_graph_free(&g);
    return;
  }
  if (B->dev_factor && w > B->dev_wmax) bj_band_coo(B, q, g.pos);
  else B->bands[q] = bj_band_rows(B, q, g.pos, w);
  if (!B->dev_factor) {
    const int bad = bj_band_cholesky(B->bands[q], b, w);
    if (bad >= 0) {
#pragma omp critical
      { if (B->fail_row < 0) B->fail_row = B->row_off + r0 + g.order[bad]; }
    }
  }
  for (int j = 0; j < b; ++j) {
    B->map_f[r0 + j] = g.order[j];
    B->map_b[r0 + j] = g.order[b - 1 - j];
  }
  bj_block_graph_free(&g);
}

/* ---- stage 2: record offsets and the device arrays of the records ----------- */
/* Narrow bands (one wavefront per block): one record of wr doubles per step,
 * [L(j+1..j+w, j) / L(j,j) | 0], wr = w + 1 rounded up to even.  Wide bands (one workgroup per
 * block): records of W = pa_bj_wide_window(w) >= w + 64 doubles in window-slot order, the value
 * for target row i at column i mod W.
 * Bands above `wide_from` get one workgroup per block (k_bj_wide) instead of one wavefront
 * (k_bj_apply / k_bj_mfma): always above 448, where the wavefront's registers end, and from
 * 97 on when the blocks are too few to give every SIMD a wavefront -- a lone wavefront per
 * SIMD is latency bound (measured on Poisson 100^3 with 512 blocks, w = 133: 1.6 ms).
 * PREALPS_BJ_WIDE_FROM = first band that is NOT given to a single wavefront, minus one
 * (tests use it to reach both dispatches on small problems).  The device factorisation lays
 * out window-slot records only for bands above pa_bj_factor_wmax(), and a wavefront's
 * registers end at 64 * maxR - 64.
 * The device arrays come first: the factors are written in place, by the factorisation kernel for
 * the narrow blocks and by per-block uploads for the ones factored on the host. */
static int bj_record_offsets(pa_bj_t* s, bj_build_t* B) {
  const int np = B->np, m = B->m, maxR = pa_bj_max_R();
  B->wide_from = np < 1024 ? pa_bj_factor_wmax() : 64 * maxR - 64;
  const char* e = getenv("PREALPS_BJ_WIDE_FROM");
  if (e && *e) {
    B->wide_from = atoi(e);
    if (B->wide_from < pa_bj_factor_wmax()) B->wide_from = pa_bj_factor_wmax();
    if (B->wide_from > 64 * maxR - 64) B->wide_from = 64 * maxR - 64;
  }
  int maxw = 0, maxw_all = 0;
  long long maxrec = 0;
  B->off[0] = 0;
  for (int q = 0; q < np; ++q) {
    const int w = B->bw[q];
    const long long reclen = w > B->wide_from ? pa_bj_wide_window(w) : ((w + 2) & ~1);
    if (w > maxw_all) maxw_all = w;
    if (B->is_nd[q]) { B->off[q + 1] = B->off[q]; ++B->nnd; continue; }     /* no band records: sparse factor */
    if (w <= B->wide_from && reclen > maxrec) maxrec = reclen;
    if (B->dev_factor) ++B->ndev;
    B->off[q + 1] = B->off[q] + (long long)B->nrows[q] * reclen;
    if (w > maxw) maxw = w;
  }
  s->max_bw = maxw_all;
  if (pa_bj_wide_window(maxw) > 4096)
    return BJ_FAIL("block-Jacobi: a diagonal block has bandwidth %d after reordering; the workgroup-resident "
                   "solve supports up to 4032 -- use more (smaller) subdomains", maxw);
  const size_t tot = B->tot = (size_t)B->off[np];
  /* A narrow block is streamed in chunks of 8 steps, whole KiB each: the last chunk of a block whose rows are no
   * multiple of 8 reads up to 7 records and 1 KiB beyond the block -- behind the last block, into this slack. */
  const size_t pad = 256 + 8 * (size_t)maxrec;
  s->d_invd_f = (double*)pa_rt_malloc((size_t)(m ? m : 1) * sizeof(double));
  s->d_invd_b = (double*)pa_rt_malloc((size_t)(m ? m : 1) * sizeof(double));
  s->d_Lf = (double*)pa_rt_malloc((tot + pad) * sizeof(double));
  s->d_Lb = (double*)pa_rt_malloc((tot + pad) * sizeof(double));
  if (!s->d_Lf || !s->d_Lb || !s->d_invd_f || !s->d_invd_b ||
      pa_rt_memset(s->d_Lf, 0, (tot + pad) * sizeof(double)) || pa_rt_memset(s->d_Lb, 0, (tot + pad) * sizeof(double)))
    return BJ_FAIL("allocating %zu factor entries on the device failed: %s", tot, pa_rt_error());
  return 0;
}

/* ---- stage 3: records of the host-factored blocks, staged upload ------------ */
/* Steps [j0, j0 + 256) of block x from its factored band into the forward / backward records f / g. */
static void bj_layout_slab(bj_build_t* B, int x, int j0, double* f, double* g) {
  const int b = B->nrows[x], w = B->bw[x], r0 = B->row0[x];
  const size_t ld = (size_t)w + 1;
  const int wide = w > B->wide_from;
  const size_t reclen = wide ? (size_t)pa_bj_wide_window(w) : (size_t)((w + 2) & ~1);
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

/* Host-factored blocks: runs of consecutive blocks (up to 64 MiB of records) are laid out
 * by the host threads into a staging buffer (256 MiB, or one block if larger) and go to
 * the device in one copy each.  Then 1 / L(j,j) of every row (the device factorisation overwrites its own). */
static int bj_layout_host(pa_bj_t* s, bj_build_t* B) {
  const int np = B->np;
  const long long* off = B->off;
  const size_t cap = (size_t)32 << 20;                   /* doubles: 256 MiB per staging buffer */
  size_t sf_cap = 0;
  double* sf = NULL; double* sg = NULL;
  int rc = 0, q = 0;
  while (B->ndev + B->nnd < np && q < np && !rc) {
    if (B->dev_factor || B->is_nd[q]) { ++q; continue; }
    int q1 = q;
    while (q1 < np && !B->dev_factor && !B->is_nd[q1] && (q1 == q || (size_t)(off[q1 + 1] - off[q]) <= cap)) ++q1;
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
    nitem = 0;
    for (int x = q; x < q1; ++x)
      for (int j0 = 0; j0 < B->nrows[x]; j0 += 256) { item_part[nitem] = x; item_j0[nitem++] = j0; }
#pragma omp parallel for num_threads(pa_host_threads()) schedule(dynamic, 4)
    for (int it = 0; it < nitem; ++it) {
      const int x = item_part[it];
      bj_layout_slab(B, x, item_j0[it], sf + (off[x] - off[q]), sg + (off[x] - off[q]));
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

/* ---- stage 4: classes by register sets, their block lists on the device ----- */
/* A narrow block of band w needs R = ceil((w + 64) / 64) register sets per lane of the one-wavefront
 * kernels; a wide one is in class -(register sets per lane of k_bj_wide).  Sparse-factored blocks are in
 * no class. */
static int bj_build_classes(pa_bj_t* s, const bj_build_t* B) {
  const int np = B->np;
  int rc = 0;
  int* cls = (int*)malloc(np * sizeof(int));
  s->nclass = 0;
  for (int q = 0; q < np; ++q) {
    int R = (B->bw[q] + 127) / 64, c;
    cls[q] = -1;
    if (B->is_nd[q]) continue;
    if (B->bw[q] > B->wide_from) { /* wide classes: -(register sets per lane) */
      int W = pa_bj_wide_window(B->bw[q]);
      R = W <= 1024 ? -1 : (W <= 2048 ? -2 : -4);
    }
    for (c = 0; c < s->nclass; ++c) if (s->class_R[c] == R) break;
    if (c == s->nclass) { s->class_R[c] = R; s->class_count[c] = 0; s->class_wmax[c] = 0; s->class_bmax[c] = 0; s->nclass++; }
    cls[q] = c; s->class_count[c]++;
    if (B->bw[q] > s->class_wmax[c]) s->class_wmax[c] = B->bw[q];
    if (B->nrows[q] > s->class_bmax[c]) s->class_bmax[c] = B->nrows[q];
  }
  for (int c = 0; c < s->nclass && !rc; ++c) {
    int* list = (int*)malloc(s->class_count[c] * sizeof(int));
    int n = 0;
    for (int q = 0; q < np; ++q) if (cls[q] == c) list[n++] = q;
    s->class_list[c] = (int*)pa_rt_malloc(n * sizeof(int));
    rc = !s->class_list[c] || pa_rt_h2d(s->class_list[c], list, n * sizeof(int));
    s->class_list_c[c] = s->class_list[c];
    free(list);
  }
  free(cls);
  if (rc) rc = BJ_FAIL("uploading block lists failed: %s", pa_rt_error());
  return rc;
}

/* ---- stage 5: the per-block and per-row index arrays ------------------------ */
static int bj_upload_index(pa_bj_t* s, const bj_build_t* B) {
  const int np = B->np, m = B->m;
  s->d_row0 = (int*)pa_rt_malloc(np * sizeof(int));
  s->d_nrows = (int*)pa_rt_malloc(np * sizeof(int));
  s->d_bw = (int*)pa_rt_malloc(np * sizeof(int));
  s->d_off = (long long*)pa_rt_malloc((np + 1) * sizeof(long long));
  s->d_map_f = (int*)pa_rt_malloc((size_t)(m ? m : 1) * sizeof(int));
  s->d_map_b = (int*)pa_rt_malloc((size_t)(m ? m : 1) * sizeof(int));
  int bad = !s->d_row0 || !s->d_nrows || !s->d_bw || !s->d_off || !s->d_map_f || !s->d_map_b;
  bad = bad || pa_rt_h2d(s->d_row0, B->row0, np * sizeof(int)) || pa_rt_h2d(s->d_nrows, B->nrows, np * sizeof(int)) ||
        pa_rt_h2d(s->d_bw, B->bw, np * sizeof(int)) || pa_rt_h2d(s->d_off, B->off, (np + 1) * sizeof(long long)) ||
        pa_rt_h2d(s->d_map_f, B->map_f, (size_t)m * sizeof(int)) || pa_rt_h2d(s->d_map_b, B->map_b, (size_t)m * sizeof(int));
  return bad ? BJ_FAIL("uploading the block factors failed: %s", pa_rt_error()) : 0;
}

/* ---- stage 6: factorisation on the device ------------------------------------ */
/* Narrow bands: runs of consecutive blocks go up in one copy of at most 256 MiB, and the host copy of a
 * band is released as soon as it is on the device. */
static int bj_upload_bands(bj_build_t* B, const long long* boff, double* d_band) {
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
static int bj_scatter_wide(const bj_build_t* B, const long long* boff, double* d_band) {
  const int np = B->np;
  int rc = 0;
  size_t ntot = 0;
  size_t* cbase = (size_t*)malloc((np + 1) * sizeof(size_t));
  for (int q = 0; q < np; ++q) { cbase[q] = ntot; ntot += B->coo_n[q]; }
  long long* go = (long long*)malloc((ntot ? ntot : 1) * sizeof(long long));
  double* gv = (double*)malloc((ntot ? ntot : 1) * sizeof(double));
  long long* d_go = (long long*)pa_rt_malloc((ntot ? ntot : 1) * sizeof(long long));
  double* d_gv = (double*)pa_rt_malloc((ntot ? ntot : 1) * sizeof(double));
  if (!go || !gv || !d_go || !d_gv) rc = BJ_FAIL("out of memory for %zu band entries", ntot);
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

/* Ship the assembled bands, factor and lay out on the device: bands up to dev_wmax with
 * the LDS-window kernel (row-major band), wider ones with the blocked kernel
 * (diagonal-major band, factored in place). */
static int bj_factor_device(pa_bj_t* s, bj_build_t* B) {
  const int np = B->np;
  int rc = 0;
  long long* boff = (long long*)malloc((np + 1) * sizeof(long long));
  int* slist = (int*)malloc(np * sizeof(int));
  int* blist = (int*)malloc(np * sizeof(int));
  size_t btot = 0;
  int ns = 0, nbig = 0, wsmall = 0, wbig = 0;
  for (int q = 0; q < np; ++q) {
    boff[q] = (long long)btot;
    if (B->is_nd[q]) continue;
    btot += (size_t)B->nrows[q] * (B->bw[q] + 1);
    if (B->bw[q] <= B->dev_wmax) { slist[ns++] = q; if (B->bw[q] > wsmall) wsmall = B->bw[q]; }
    else { blist[nbig++] = q; if (B->bw[q] > wbig) wbig = B->bw[q]; }
  }
  boff[np] = (long long)btot;
  double* d_band = (double*)pa_rt_malloc((btot ? btot : 1) * sizeof(double));
  long long* d_boff = (long long*)pa_rt_malloc((np + 1) * sizeof(long long));
  int* d_slist = (int*)pa_rt_malloc((ns ? ns : 1) * sizeof(int));
  int* d_blist = (int*)pa_rt_malloc((nbig ? nbig : 1) * sizeof(int));
  int* d_fail = (int*)pa_rt_malloc(sizeof(int));
  int fail = 0;
  if (!d_band || !d_boff || !d_slist || !d_blist || !d_fail)
    rc = BJ_FAIL("allocating %zu band entries on the device failed: %s", btot, pa_rt_error());
  const int tr = getenv("PREALPS_SETUP_TRACE") != NULL;
  double t_tr = pa_wtime();
  if (!rc && nbig > 0 && pa_rt_memset(d_band, 0, btot * sizeof(double))) rc = BJ_FAIL("%s", pa_rt_error());
  if (!rc) rc = bj_upload_bands(B, boff, d_band);
  if (!rc && nbig > 0) rc = bj_scatter_wide(B, boff, d_band);
  if (tr) { fprintf(stderr, "[setup] band upload (%.1f GB)        %.3f s\n", 8e-9 * (double)btot, pa_wtime() - t_tr); t_tr = pa_wtime(); }
  if (!rc) {
    if (pa_rt_h2d(d_boff, boff, (np + 1) * sizeof(long long)) || pa_rt_h2d(d_slist, slist, ns * sizeof(int)) ||
        pa_rt_h2d(d_blist, blist, nbig * sizeof(int)) || pa_rt_h2d(d_fail, &fail, sizeof(int)) ||
        pa_k_bj_factor(d_slist, ns, wsmall, s->d_row0, s->d_nrows, s->d_bw, s->d_off, d_boff, d_band, s->d_Lf,
                       s->d_Lb, s->d_invd_f, s->d_invd_b, d_fail) ||
        pa_k_bj_factor_big(d_blist, nbig, wbig, B->wide_from, s->d_row0, s->d_nrows, s->d_bw, s->d_off, d_boff,
                           d_band, s->d_Lf, s->d_Lb, s->d_invd_f, s->d_invd_b, d_fail) ||
        pa_rt_d2h(&fail, d_fail, sizeof(int)))
      rc = BJ_FAIL("factorising the diagonal blocks on the device failed: %s", pa_rt_error());
    else if (fail > 0)
      rc = BJ_FAIL("diagonal block is not SPD (global row %d)", B->row_off + B->map_f[fail - 1] +
                   B->row0[part_of_local_row(B->row0, B->nrows, np, fail - 1)]);
  }
  if (tr) fprintf(stderr, "[setup] device factorisation + layout  %.3f s\n", pa_wtime() - t_tr);
  pa_rt_free(d_band); pa_rt_free(d_boff); pa_rt_free(d_slist); pa_rt_free(d_blist); pa_rt_free(d_fail);
  free(boff); free(slist); free(blist);
  return rc;
}

/* ---- stage 7: the sparse-factored blocks go to nd.c -------------------------- */
static int bj_nd_handoff(const bj_build_t* B) {
  const int np = B->np;
  int rc = 0;
  int* ndl = (int*)malloc((size_t)B->nnd * sizeof(int));
  int* grow0 = (int*)malloc((size_t)np * sizeof(int));
  int x = 0, nd_fail = -1;
  for (int q = 0; q < np; ++q) { grow0[q] = B->rowPos[B->op->part0 + q]; if (B->is_nd[q]) ndl[x++] = q; }
  int r2 = pa_nd_create(B->A, B->nnd, ndl, B->row0, B->nrows, grow0, B->m, B->nd_bits, &nd_fail);
  if (r2 == 2) rc = BJ_FAIL("diagonal block is not SPD (global row %d)", B->row_off + nd_fail);
  else if (r2) rc = 1;
  free(ndl); free(grow0);
  return rc;
}

/* ---- stage 8: second layouts -------------------------------------------------- */
/* tot2 elements of 8 or 4 bytes (off2 counts elements: every offset a multiple of 8 of them, so a block
 * starts 32-byte aligned in fp32 too), and 8 KiB of zeroed slack: a request of the apply reads whole KiB
 * from a chunk's start, up to 1 KiB beyond the end of the last block's last chunk. */
/* The launches that fill the second layouts from the plain records (the create, and the refactorisation in place). */
static int bj_launch_g4(const pa_bj_t* s) {
  for (int c = 0; c < s->nclass; ++c)
    if (s->class_g4[c] &&
        (s->g4_bits == 32
           ? pa_k_bj_g4_setup_f32(s->class_list[c], s->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lf, (float*)s->d_Lg4)
           : pa_k_bj_g4_setup(s->class_list[c], s->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lf, (double*)s->d_Lg4)))
      return 1;
  return 0;
}

static int bj_launch_pairs(const pa_bj_t* s, const int* cls_pairs) {
  for (int c = 0; c < s->nclass; ++c)
    if (cls_pairs[c])
      if (pa_k_bj_pairs(s->class_list[c], s->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lf, s->d_Lf2) ||
          pa_k_bj_pairs(s->class_list[c], s->class_count[c], s->d_nrows, s->d_bw, s->d_off, s->d_off2, s->d_Lb, s->d_Lb2))
        return 1;
  return 0;
}

static int bj_make_g4(pa_bj_t* s, int band_bits, long long tot2) {
  const size_t esz = band_bits == 32 ? sizeof(float) : sizeof(double);
  const size_t g4_alloc = (size_t)tot2 * esz + 8192;
  s->g4_bits = band_bits;
  s->d_Lg4 = pa_rt_malloc(g4_alloc);
  if (!s->d_Lg4 || pa_rt_memset(s->d_Lg4, 0, g4_alloc))
    return BJ_FAIL("allocating the one-copy sweep records failed: %s", pa_rt_error());
  if (bj_launch_g4(s)) return BJ_FAIL("k_bj_g4_setup failed");
  s->g4_bytes = (double)esz * (double)tot2;
  return 0;
}

static int bj_make_pairs(pa_bj_t* s, const int* cls_pairs, long long tot2) {
  s->d_Lf2 = (double*)pa_rt_malloc(((size_t)tot2 + 1024) * sizeof(double));
  s->d_Lb2 = (double*)pa_rt_malloc(((size_t)tot2 + 1024) * sizeof(double));
  if (!s->d_Lf2 || !s->d_Lb2 ||
      pa_rt_memset(s->d_Lf2 + tot2, 0, 512 * sizeof(double)) || pa_rt_memset(s->d_Lb2 + tot2, 0, 512 * sizeof(double)))
    return BJ_FAIL("allocating the paired sweep records failed: %s", pa_rt_error());
  if (bj_launch_pairs(s, cls_pairs)) return BJ_FAIL("k_bj_pairs failed");
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
 * the 8- and 16-column kernels. */
static int bj_second_layouts(pa_bj_t* s, const bj_build_t* B) {
  const int np = B->np;
  const int want_g4 = !(getenv("PREALPS_BJ_G4") && atoi(getenv("PREALPS_BJ_G4")) == 0) && (long long)B->m * 16 < 2147483647LL;
  const int want_pairs = !(getenv("PREALPS_BJ_PAIRS") && atoi(getenv("PREALPS_BJ_PAIRS")) == 0);
  int rc = 0, any_g4 = 0, any_pairs = 0, cls_pairs[16];
  for (int c = 0; c < s->nclass; ++c) {
    s->class_g4[c] = want_g4 && s->class_R[c] > 0 && s->class_wmax[c] <= pa_bj_g4_max_band() &&
                      s->class_bmax[c] <= pa_bj_g4_max_rows();
    cls_pairs[c] = want_pairs && !s->class_g4[c] && (s->class_R[c] == 2 || s->class_R[c] == 3);
    any_g4 |= s->class_g4[c]; any_pairs |= cls_pairs[c];
    s->class_pairs[c] = cls_pairs[c];
  }
  long long* off2 = (long long*)calloc((size_t)np + 1, sizeof(long long));
  long long tot2 = 0;
  if (off2 && (any_g4 || any_pairs)) {
    for (int q = 0; q < np; ++q) {
      if (B->is_nd[q] || B->bw[q] > B->wide_from) continue;
      off2[q] = tot2;                                   /* (blocks of the other classes: unused) */
      tot2 += 8LL * ((B->nrows[q] + 7) / 8) * (B->bw[q] + 4);
    }
    s->d_off2 = (long long*)pa_rt_malloc(((size_t)np + 1) * sizeof(long long));
    if (!s->d_off2 || pa_rt_h2d(s->d_off2, off2, ((size_t)np + 1) * sizeof(long long)))
      rc = BJ_FAIL("allocating the second sweep records failed: %s", pa_rt_error());
    if (!rc && any_g4) rc = bj_make_g4(s, B->band_bits, tot2);
    if (!rc && any_pairs) rc = bj_make_pairs(s, cls_pairs, tot2);
    if (!rc && pa_rt_sync()) rc = BJ_FAIL("%s", pa_rt_error());
  }
  free(off2);
  return rc;
}

/* ---- stage 9: the plan the kernels read, from the arrays pa_bj_t owns ------- */
static void bj_fill_plan(pa_bj_t* s) {
  pa_bj_plan_t* pl = &s->plan;
  pl->nparts = s->np; pl->row0 = s->d_row0; pl->nrows = s->d_nrows; pl->bw = s->d_bw; pl->off = s->d_off;
  pl->map_f = s->d_map_f; pl->map_b = s->d_map_b; pl->Lf = s->d_Lf; pl->Lb = s->d_Lb;
  pl->invd_f = s->d_invd_f; pl->invd_b = s->d_invd_b;
  pl->Lf2 = s->d_Lf2; pl->Lb2 = s->d_Lb2; pl->off2 = s->d_off2;
  pl->Lg4 = s->d_Lg4; pl->g4_bits = s->d_Lg4 ? s->g4_bits : 0; pl->class_g4 = s->class_g4; pl->class_bmax = s->class_bmax;
  pl->nclass = s->nclass; pl->class_R = s->class_R; pl->class_count = s->class_count;
  pl->class_wmax = s->class_wmax;
  pl->class_list = s->class_list_c;
}

/* ---- stage 10: what a later preAlps_BlockJacobiUpdateValues needs (host memory only) ---- */
static void* bj_dup(const void* p, size_t bytes) {
  void* c = malloc(bytes ? bytes : 1);
  if (c) memcpy(c, p, bytes);
  return c;
}

static int bj_keep_decisions(pa_bj_t* s, const bj_build_t* B) {
  const size_t np = (size_t)B->np;
  s->h_row0 = (int*)bj_dup(B->row0, np * sizeof(int));
  s->h_nrows = (int*)bj_dup(B->nrows, np * sizeof(int));
  s->h_bw = (int*)bj_dup(B->bw, np * sizeof(int));
  s->h_is_nd = (char*)bj_dup(B->is_nd, np);
  s->h_map_f = (int*)bj_dup(B->map_f, (size_t)B->m * sizeof(int));
  s->h_grow0 = (int*)bj_dup(B->rowPos + B->op->part0, np * sizeof(int));
  if (!s->h_row0 || !s->h_nrows || !s->h_bw || !s->h_is_nd || !s->h_map_f || !s->h_grow0)
    return BJ_FAIL("out of host memory for the block arrays");
  s->row_off = B->row_off; s->wide_from = B->wide_from; s->dev_factor = B->dev_factor; s->dev_wmax = B->dev_wmax;
  s->nd_bits = B->nd_bits; s->tot = B->tot;
  s->A_rowptr = B->A->rowPtr; s->op_build = pa_operator_build_count();
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
  /* band blocks stay fp64 but for the one-copy records of bj_g4.hip */
  int nd_bits, band_bits;
  if (bj_storage_bits(g_nd_bits, "PREALPS_BJ_ND_PRECISION", "sparse block factors", &nd_bits) ||
      bj_storage_bits(g_band_bits, "PREALPS_BJ_BAND_PRECISION", "one-copy band records", &band_bits))
    return 1;
  if (g_bj.created) preAlps_BlockJacobiFree();
  pa_bj_t* s = &g_bj;
  bj_build_t B;
  bj_build_init(&B, A, rowPos, op);
  B.nd_bits = nd_bits; B.band_bits = band_bits;
  s->np = B.np; s->m = B.m;

  double t_setup0 = pa_wtime();
  /* pass 1 (parallel over blocks): RCM order, bandwidth, band assembly, host band Cholesky */
#pragma omp parallel for num_threads(pa_host_threads()) schedule(dynamic, 1)
  for (int q = 0; q < B.np; ++q) bj_host_block(&B, q);
  int rc = 0;
  g_bj_setup_s[0] = pa_wtime() - t_setup0;
  t_setup0 = pa_wtime();
  if (B.fail_row >= 0) rc = PA_FAIL("diagonal block is not SPD (global row %d)", B.fail_row);
  /* pass 2: sweep layouts, in this order (device allocations, uploads and syncs follow it) */
  if (!rc) rc = bj_record_offsets(s, &B);
  if (!rc) rc = bj_layout_host(s, &B);
  if (!rc) rc = bj_build_classes(s, &B);
  if (!rc) rc = bj_upload_index(s, &B);
  if (!rc && B.ndev > 0) rc = bj_factor_device(s, &B);
  if (!rc && B.nnd > 0) rc = bj_nd_handoff(&B);
  if (!rc) rc = bj_second_layouts(s, &B);
  if (!rc) rc = bj_keep_decisions(s, &B);
  const size_t tot = B.tot;
  const int nnd = B.nnd;
  bj_build_release(&B);
  if (rc) { preAlps_BlockJacobiFree(); return rc; }
  s->factor_bytes = 2.0 * 8.0 * (double)tot + pa_nd_factor_bytes();
  s->nd_blocks = nnd;
  bj_fill_plan(s);
  s->created = 1;
  ++g_bj_apply_epoch;
  g_bj_values_epoch = pa_operator_values_epoch();
  g_bj_setup_s[1] = pa_wtime() - t_setup0;
  return 0;
}

/* ---- coarse space: M^-1 = B^-1 + Z E^-1 Z^T (coarse_space.c on the host, coarse.hip on the device) ------------ */
#define BJC_FAIL(...) pa_fail_at("preAlps_BlockJacobiSetCoarseSpace", __VA_ARGS__)

/* zv, the chunk lists, E and Einv on the host from the vectors and aggregates in `co` and the operator's current panel,
 * permutation and scaling: Vp = (D^-1 V)[perm].  The reason of a failure goes to err. */
static int bj_coarse_host(const pa_bj_t* s, const pa_bj_coarse_t* co, const pa_operator_info_t* op, pa_coarse_t* hc,
                          char* err, size_t errlen) {
  const int m = op->m, k = co->k, np = s->np;
  double* Vp = (double*)malloc(((size_t)m * k + 1) * sizeof(double));
  int* rp = (int*)malloc(((size_t)np + 1) * sizeof(int));
  if (!Vp || !rp) { free(Vp); free(rp); snprintf(err, errlen, "out of host memory"); return PA_COARSE_NOMEM; }
  for (int q = 0; q <= np; ++q) rp[q] = op->rowPos[op->part0 + q] - op->row_off;
#pragma omp parallel for num_threads(pa_host_threads()) schedule(static)
  for (int i = 0; i < m; ++i) {
    const int old = op->perm[op->row_off + i];
    const double d = op->scaling ? op->scaling[old] : 1.0;
    for (int a = 0; a < k; ++a) Vp[(size_t)i * k + a] = co->V[(size_t)a * co->n + old] / d;
  }
  pa_coarse_in_t in = {.m = m, .nparts = np, .rowPtr = op->A.rowPtr, .lcol = op->A.colInd, .val = op->A.val, .rowPos = rp,
                       .part_aggregate = co->part_aggregate, .naggr = co->naggr, .k = k, .Vp = Vp,
                       .max_dofs = PA_COARSE_MAX_DOFS, .threads = pa_host_threads()};
  const int rc = pa_coarse_build(&in, hc, err, errlen);
  free(Vp); free(rp);
  return rc;
}

int preAlps_BlockJacobiClearCoarseSpace(void) {
  pa_bj_t* s = &g_bj;
  if (s->co.on && pa_rt_sync()) return pa_fail_at(__func__, "%s", pa_rt_error());
  bj_coarse_release(&s->co);
  ++g_bj_apply_epoch;
  return 0;
}

/* part_aggregate[p] of the attached coarse space for the np local parts (the caller's, or the default the library
 * chose); *naggr (may be NULL) the number of aggregates */
int preAlps_BlockJacobiGetCoarseAggregates(int* part_aggregate, int* naggr) {
  const pa_bj_t* s = &g_bj;
  if (!s->created || !s->co.on) return pa_fail_at(__func__, "no coarse space attached");
  if (!part_aggregate) return pa_fail_at(__func__, " wrong test 'part_aggregate != NULL'");
  memcpy(part_aggregate, s->co.part_aggregate, (size_t)s->np * sizeof(int));
  if (naggr) *naggr = s->co.naggr;
  return 0;
}

int preAlps_BlockJacobiSetCoarseSpace(int k, const double* V, int ldv, const int* part_aggregate, int naggr) {
  pa_bj_t* s = &g_bj;
  const double t0 = pa_wtime();
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return BJC_FAIL("operator not built");
  if (k < 1 || k > PA_COARSE_MAX_VECS) return BJC_FAIL("k = %d vectors refused: 1 .. %d", k, PA_COARSE_MAX_VECS);
  if (!V) return BJC_FAIL(" wrong test 'V != NULL'");
  const int N = op->N;
  if (ldv < N) return BJC_FAIL("ldv = %d is smaller than the %d rows of the matrix", ldv, N);
  for (int a = 0; a < k; ++a)
    for (int i = 0; i < N; ++i)
      if (!isfinite(V[(size_t)a * ldv + i])) return BJC_FAIL("V(%d, %d) is not finite", i, a);
  if (part_aggregate && (long long)naggr * k > PA_COARSE_MAX_DOFS)
    return BJC_FAIL("%d aggregates x %d vectors = %lld coarse unknowns, the cap is %d", naggr, k, (long long)naggr * k,
                    PA_COARSE_MAX_DOFS);
  if (part_aggregate && naggr < 1) return BJC_FAIL("naggr = %d refused", naggr);
  if (pa_operator_plan_only()) return BJC_FAIL("the operator was built in plan-only mode (no GPU)");
  if (pa_world_size() > 1 || pa_comm_is_loopback())
    return BJC_FAIL("the coarse space is for one process (%d processes%s)", pa_world_size(),
                    pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "");
  if (!s->created) return BJC_FAIL("preconditioner not created");
  if (pa_operator_build_count() != s->op_build || s->A_rowptr != op->A.rowPtr)
    return BJC_FAIL("the preconditioner was not created from the current operator's own panel");

  pa_bj_coarse_t co;
  memset(&co, 0, sizeof(co));
  char err[320];
  err[0] = 0;
  int rc = 0;
  const int np = s->np;
  co.k = k; co.n = N;
  co.V = (double*)malloc((size_t)N * k * sizeof(double));
  co.part_aggregate = (int*)malloc((size_t)np * sizeof(int));
  if (!co.V || !co.part_aggregate) { bj_coarse_release(&co); return BJC_FAIL("out of host memory for the %d vectors", k); }
  for (int a = 0; a < k; ++a) memcpy(co.V + (size_t)a * N, V + (size_t)a * ldv, (size_t)N * sizeof(double));
  if (part_aggregate) {
    memcpy(co.part_aggregate, part_aggregate, (size_t)np * sizeof(int));
    co.naggr = naggr;
  } else {
    int* rp = (int*)malloc(((size_t)np + 1) * sizeof(int));
    if (!rp) { bj_coarse_release(&co); return BJC_FAIL("out of host memory"); }
    for (int q = 0; q <= np; ++q) rp[q] = op->rowPos[op->part0 + q] - op->row_off;
    pa_coarse_in_t in = {.m = op->m, .nparts = np, .rowPtr = op->A.rowPtr, .lcol = op->A.colInd, .val = op->A.val,
                         .rowPos = rp, .k = k, .max_dofs = PA_COARSE_MAX_DOFS};
    rc = pa_coarse_default_aggregates(&in, preAlps_hip_partition_kway, co.part_aggregate, &co.naggr, err, sizeof(err));
    free(rp);
    if (rc) { bj_coarse_release(&co); return BJC_FAIL("default aggregates: %s", err[0] ? err : preAlps_hip_last_error()); }
  }
  pa_coarse_t hc;
  rc = bj_coarse_host(s, &co, op, &hc, err, sizeof(err));
  if (rc) { bj_coarse_release(&co); return BJC_FAIL("%s", err); }
  co.naggr = hc.naggr; co.nc = hc.nc; co.nchunks = hc.nchunks;
  const size_t m = (size_t)op->m, nch = (size_t)hc.nchunks, nn = (size_t)hc.nc * hc.nc;
  const size_t b_zv = m * k * sizeof(double), b_ch = nch * sizeof(int), b_ap = ((size_t)hc.naggr + 1) * sizeof(int),
               b_ei = nn * sizeof(double), b_pa = nch * k * 16 * sizeof(double), b_cy = (size_t)hc.nc * 16 * sizeof(double);
  co.d_zv = (double*)pa_rt_malloc(b_zv);
  co.d_ch_row0 = (int*)pa_rt_malloc(b_ch); co.d_ch_nrows = (int*)pa_rt_malloc(b_ch); co.d_ch_aggr = (int*)pa_rt_malloc(b_ch);
  co.d_agg_ptr = (int*)pa_rt_malloc(b_ap); co.d_agg_chunk = (int*)pa_rt_malloc(b_ch);
  co.d_Einv = (double*)pa_rt_malloc(b_ei); co.d_partial = (double*)pa_rt_malloc(b_pa);
  co.d_c = (double*)pa_rt_malloc(b_cy); co.d_y = (double*)pa_rt_malloc(b_cy);
  if (!co.d_zv || !co.d_ch_row0 || !co.d_ch_nrows || !co.d_ch_aggr || !co.d_agg_ptr || !co.d_agg_chunk || !co.d_Einv ||
      !co.d_partial || !co.d_c || !co.d_y ||
      pa_rt_h2d(co.d_zv, hc.zv, b_zv) || pa_rt_h2d(co.d_ch_row0, hc.ch_row0, b_ch) || pa_rt_h2d(co.d_ch_nrows, hc.ch_nrows, b_ch) ||
      pa_rt_h2d(co.d_ch_aggr, hc.ch_aggr, b_ch) || pa_rt_h2d(co.d_agg_ptr, hc.agg_ptr, b_ap) ||
      pa_rt_h2d(co.d_agg_chunk, hc.agg_chunk, b_ch) || pa_rt_h2d(co.d_Einv, hc.Einv, b_ei) ||
      pa_rt_memset(co.d_partial, 0, b_pa) || pa_rt_memset(co.d_c, 0, b_cy) || pa_rt_memset(co.d_y, 0, b_cy) || pa_rt_sync()) {
    pa_coarse_free(&hc);
    bj_coarse_release(&co);
    return BJC_FAIL("uploading the coarse space (%zu bytes of Einv) failed: %s", b_ei, pa_rt_error());
  }
  pa_coarse_free(&hc);
  co.bytes = (double)(b_zv + 4 * b_ch + b_ap + b_ei + b_pa + 2 * b_cy);
  co.plan = (pa_coarse_plan_t){.m = op->m, .k = k, .naggr = co.naggr, .nc = co.nc, .nchunks = co.nchunks, .zv = co.d_zv,
                               .ch_row0 = co.d_ch_row0, .ch_nrows = co.d_ch_nrows, .ch_aggr = co.d_ch_aggr,
                               .agg_ptr = co.d_agg_ptr, .agg_chunk = co.d_agg_chunk, .Einv = co.d_Einv,
                               .partial = co.d_partial, .c = co.d_c, .y = co.d_y};
  co.on = 1; co.builds = 1;
  co.setup_s = pa_wtime() - t0;
  bj_coarse_release(&s->co);        /* setting a coarse space again replaces it (the copies above have drained the stream) */
  s->co = co;
  ++g_bj_apply_epoch;
  return 0;
}

/* ---- numeric refactorisation in place (preAlps_BlockJacobiUpdateValues) ---------- */
#define BJU_FAIL(...) pa_fail_at("preAlps_BlockJacobiUpdateValues", __VA_ARGS__)

/* The coarse space follows the new values and the new scaling vector: zv, E and Einv formed again from the kept V and
 * aggregates and written into the same device arrays (the chunk lists depend on the partition alone).  A singular E
 * drops the coarse space; the block factor is not touched here. */
static int bj_coarse_refresh(pa_bj_t* s, const pa_operator_info_t* op) {
  pa_bj_coarse_t* co = &s->co;
  const double t0 = pa_wtime();
  char err[320];
  err[0] = 0;
  pa_coarse_t hc;
  int rc = bj_coarse_host(s, co, op, &hc, err, sizeof(err));
  if (!rc && (hc.nc != co->nc || hc.nchunks != co->nchunks)) { rc = 1; snprintf(err, sizeof(err), "the partition changed"); pa_coarse_free(&hc); }
  if (rc) {
    if (pa_rt_sync()) { /* nothing more to report */ }
    bj_coarse_release(co);
    ++g_bj_apply_epoch;
    return BJU_FAIL("the coarse space was dropped, the refreshed block factor stays: %s", err);
  }
  if (pa_rt_h2d(co->d_zv, hc.zv, (size_t)op->m * co->k * sizeof(double)) ||
      pa_rt_h2d(co->d_Einv, hc.Einv, (size_t)hc.nc * hc.nc * sizeof(double))) {
    pa_coarse_free(&hc);
    bj_coarse_release(co);
    ++g_bj_apply_epoch;
    return BJU_FAIL("the coarse space was dropped: uploading it failed: %s", pa_rt_error());
  }
  pa_coarse_free(&hc);
  ++co->builds;
  co->setup_s = pa_wtime() - t0;
  return 0;
}

/* The band map of the current preconditioner on the device, with the offsets of the bands and the launch lists of
 * pa_k_bj_factor / pa_k_bj_factor_big as bj_factor_device forms them: cut once per create. */
static int bj_ensure_band_map(pa_bj_t* s, const pa_operator_info_t* op) {
  if (s->d_bm_src) return 0;
  const int np = s->np;
  const double t0 = pa_wtime();
  pa_bj_band_map_in_t in = {.np = np, .rowPtr = op->A.rowPtr, .colInd = op->A.colInd, .row0 = s->h_row0, .nrows = s->h_nrows,
                            .grow0 = s->h_grow0, .bw = s->h_bw, .order = s->h_map_f, .is_nd = s->h_is_nd,
                            .wmax = s->dev_wmax, .chunk = 1024};
  pa_bj_band_map_t bm;
  const int brc = pa_bj_band_map_build(&in, &bm);
  if (brc == -2)
    return BJU_FAIL("the band of block %d (%d rows, bandwidth %d) has 2^32 entries or more: free and create instead",
                    bm.bad_block, s->h_nrows[bm.bad_block], s->h_bw[bm.bad_block]);
  if (brc == -3) return BJU_FAIL("block %d of the panel no longer has the pattern the preconditioner was created from", bm.bad_block);
  if (brc) return BJU_FAIL("out of host memory for the band map");
  ++s->bm_builds;
  int* slist = (int*)malloc((np ? np : 1) * sizeof(int));
  int* blist = (int*)malloc((np ? np : 1) * sizeof(int));
  int rc = 0;
  if (!slist || !blist) rc = BJU_FAIL("out of host memory for the band map");
  s->ns = s->nbig = s->wsmall = s->wbig = 0;
  for (int q = 0; q < np && !rc; ++q) {
    if (s->h_is_nd[q]) continue;
    if (s->h_bw[q] <= s->dev_wmax) { slist[s->ns++] = q; if (s->h_bw[q] > s->wsmall) s->wsmall = s->h_bw[q]; }
    else { blist[s->nbig++] = q; if (s->h_bw[q] > s->wbig) s->wbig = s->h_bw[q]; }
  }
  if (!rc) {
    s->d_bm_src = (unsigned*)pa_rt_malloc((bm.n ? bm.n : 1) * sizeof(unsigned));
    s->d_bm_dst = (unsigned*)pa_rt_malloc((bm.n ? bm.n : 1) * sizeof(unsigned));
    s->d_bm_chunk_blk = (int*)pa_rt_malloc((bm.nchunks ? bm.nchunks : 1) * sizeof(int));
    s->d_bm_chunk_first = (unsigned*)pa_rt_malloc((bm.nchunks + 1) * sizeof(unsigned));
    s->d_boff = (long long*)pa_rt_malloc(((size_t)np + 1) * sizeof(long long));
    s->d_slist = (int*)pa_rt_malloc((s->ns ? s->ns : 1) * sizeof(int));
    s->d_blist = (int*)pa_rt_malloc((s->nbig ? s->nbig : 1) * sizeof(int));
    s->d_fail = (int*)pa_rt_malloc(sizeof(int));
    if (!s->d_bm_src || !s->d_bm_dst || !s->d_bm_chunk_blk || !s->d_bm_chunk_first || !s->d_boff || !s->d_slist ||
        !s->d_blist || !s->d_fail ||
        pa_rt_h2d(s->d_bm_src, bm.src, bm.n * sizeof(unsigned)) || pa_rt_h2d(s->d_bm_dst, bm.dst, bm.n * sizeof(unsigned)) ||
        pa_rt_h2d(s->d_bm_chunk_blk, bm.chunk_blk, bm.nchunks * sizeof(int)) ||
        pa_rt_h2d(s->d_bm_chunk_first, bm.chunk_first, (bm.nchunks + 1) * sizeof(unsigned)) ||
        pa_rt_h2d(s->d_boff, bm.boff, ((size_t)np + 1) * sizeof(long long)) ||
        pa_rt_h2d(s->d_slist, slist, (size_t)s->ns * sizeof(int)) || pa_rt_h2d(s->d_blist, blist, (size_t)s->nbig * sizeof(int))) {
      rc = BJU_FAIL("uploading the band map (%zu entries) failed: %s", bm.n, pa_rt_error());
      pa_rt_free(s->d_bm_src); pa_rt_free(s->d_bm_dst); pa_rt_free(s->d_bm_chunk_blk); pa_rt_free(s->d_bm_chunk_first);
      pa_rt_free(s->d_boff); pa_rt_free(s->d_slist); pa_rt_free(s->d_blist); pa_rt_free(s->d_fail);
      s->d_bm_src = s->d_bm_dst = s->d_bm_chunk_first = NULL; s->d_bm_chunk_blk = s->d_slist = s->d_blist = s->d_fail = NULL;
      s->d_boff = NULL;
    }
  }
  if (!rc) {
    s->bm_n = bm.n; s->bm_nchunks = bm.nchunks; s->bm_bytes = pa_bj_band_map_bytes(&bm); s->btot = (size_t)bm.boff[np];
    s->upd_map_s = pa_wtime() - t0;
  }
  free(slist); free(blist);
  pa_bj_band_map_free(&bm);
  return rc;
}

/* The band blocks: panel values up in one copy, bands assembled on the device through the map, then the
 * factorisation and layout launches of the create on the create's lists, offsets and records.  Every kernel
 * writes, for the same (rows, bandwidth, wide), the positions it wrote at the create -- k_bj_factor and
 * k_bj_layout_big the in-band entries of the plain records, k_bj_g4_setup and k_bj_pairs every element of a
 * block's second record -- so the zero background of the create survives and nothing is cleared.
 * *spd_fail: 1 + local position of a non-positive pivot.  Returns non-zero with the error reported;
 * *wrote tells whether the factor may have been written to by then. */
static int bj_refactor_bands(pa_bj_t* s, const pa_operator_info_t* op, int* wrote, int* spd_fail) {
  const size_t lnnz = (size_t)op->A.rowPtr[s->m];
  double* d_pv = (double*)pa_rt_malloc((lnnz ? lnnz : 1) * sizeof(double));
  double* d_band = (double*)pa_rt_malloc((s->btot ? s->btot : 1) * sizeof(double));
  void* e0 = pa_rt_event_create();
  void* e1 = pa_rt_event_create();
  int rc = 0, fail = 0;
  if (!d_pv || !d_band || !e0 || !e1)
    rc = BJU_FAIL("no device memory for the panel values (%zu) and the bands (%zu entries): %s", lnnz, s->btot, pa_rt_error());
  if (!rc) {
    /* behind the applies already queued on the library stream; the copy returns when it has read A->val */
    const double t0 = pa_wtime();
    if (pa_rt_h2d(d_pv, op->A.val, lnnz * sizeof(double))) rc = BJU_FAIL("uploading the panel values failed: %s", pa_rt_error());
    s->upd_copy_s = pa_wtime() - t0;
  }
  if (!rc) {
    *wrote = 1;
    if (pa_rt_event_record(e0) || pa_rt_memset(d_band, 0, s->btot * sizeof(double)) || pa_rt_memset(s->d_fail, 0, sizeof(int)) ||
        pa_k_bj_band_assemble(s->d_bm_src, s->d_bm_dst, s->d_bm_chunk_blk, s->d_bm_chunk_first, s->bm_nchunks, s->d_boff,
                              d_pv, d_band) ||
        pa_k_bj_factor(s->d_slist, s->ns, s->wsmall, s->d_row0, s->d_nrows, s->d_bw, s->d_off, s->d_boff, d_band, s->d_Lf,
                       s->d_Lb, s->d_invd_f, s->d_invd_b, s->d_fail) ||
        pa_k_bj_factor_big(s->d_blist, s->nbig, s->wbig, s->wide_from, s->d_row0, s->d_nrows, s->d_bw, s->d_off, s->d_boff,
                           d_band, s->d_Lf, s->d_Lb, s->d_invd_f, s->d_invd_b, s->d_fail) ||
        pa_rt_d2h(&fail, s->d_fail, sizeof(int)))
      rc = BJU_FAIL("factorising the diagonal blocks on the device failed: %s", pa_rt_error());
    *spd_fail = fail;
  }
  if (!rc && fail == 0) {     /* the second layouts, from the new plain records */
    if (s->d_Lg4 && bj_launch_g4(s)) rc = BJU_FAIL("k_bj_g4_setup failed");
    if (!rc && s->d_Lf2 && bj_launch_pairs(s, s->class_pairs)) rc = BJU_FAIL("k_bj_pairs failed");
    if (!rc && (pa_rt_event_record(e1) || pa_rt_sync())) rc = BJU_FAIL("%s", pa_rt_error());
    if (!rc) s->upd_kernel_s = pa_rt_event_elapsed_s(e0, e1);
  }
  pa_rt_event_destroy(e0); pa_rt_event_destroy(e1);
  pa_rt_free(d_pv); pa_rt_free(d_band);
  return rc;
}

int preAlps_BlockJacobiUpdateValues(void) {
  pa_bj_t* s = &g_bj;
  const double t_all = pa_wtime();
  if (!s->created) return BJU_FAIL("preconditioner not created");
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return BJU_FAIL("operator not built: it was freed since preAlps_BlockJacobiCreate (free and create instead)");
  if (pa_operator_build_count() != s->op_build)
    return BJU_FAIL("the operator was built again since preAlps_BlockJacobiCreate: free and create instead");
  if (s->A_rowptr != op->A.rowPtr)
    return BJU_FAIL("the preconditioner was not created from the operator's own panel (preAlps_OperatorGetA): free and create instead");
  if (!s->dev_factor)
    return BJU_FAIL("the preconditioner was created with PREALPS_BJ_FACTOR=host, its records come from the host "
                    "Cholesky: free and create instead");
  int rc = 0, wrote = 0, spd_fail = 0;
  s->upd_copy_s = s->upd_kernel_s = 0.0;
  if (s->np - s->nd_blocks > 0) {
    rc = bj_ensure_band_map(s, op);
    if (rc) return rc;                      /* (nothing of the factor has been touched) */
    rc = bj_refactor_bands(s, op, &wrote, &spd_fail);
    if (!rc && spd_fail > 0)
      rc = BJU_FAIL("diagonal block is not SPD (global row %d)", s->row_off + s->h_map_f[spd_fail - 1] +
                    s->h_row0[part_of_local_row(s->h_row0, s->h_nrows, s->np, spd_fail - 1)]);
    if (rc && !wrote) return rc;
  }
  /* the blocks with the sparse factor: created again from the new panel, with the arguments of the create */
  if (!rc && s->nd_blocks > 0) {
    int* ndl = (int*)malloc((size_t)s->nd_blocks * sizeof(int));
    int x = 0, nd_fail = -1;
    if (!ndl) rc = BJU_FAIL("out of host memory");
    else {
      for (int q = 0; q < s->np; ++q) if (s->h_is_nd[q]) ndl[x++] = q;
      const int r2 = pa_nd_create(&op->A, s->nd_blocks, ndl, s->h_row0, s->h_nrows, s->h_grow0, s->m, s->nd_bits, &nd_fail);
      if (r2 == 2) rc = BJU_FAIL("diagonal block is not SPD (global row %d)", s->row_off + nd_fail);
      else if (r2) rc = 1;
      else { s->nd_rebuilt = s->nd_blocks; s->factor_bytes = 2.0 * 8.0 * (double)s->tot + pa_nd_factor_bytes(); }
      free(ndl);
    }
  }
  /* the records hold the new values in part, or not even a factor: there is no old preconditioner to go back to */
  if (rc) { preAlps_BlockJacobiFree(); return rc; }
  ++s->updates;
  g_bj_values_epoch = pa_operator_values_epoch();
  if (s->co.on) rc = bj_coarse_refresh(s, op);
  s->upd_total_s = pa_wtime() - t_all;
  return rc;
}

/* "bj_updates", "bj_band_map_*", "bj_update_*", the two addresses: preAlps_hip_get_stat; 0 = key known */
int pa_bj_update_stat(const char* key, double* value) {
  const pa_bj_t* s = &g_bj;
  const int on = s->created;
  if (!strcmp(key, "bj_updates")) *value = on ? s->updates : 0;
  else if (!strcmp(key, "bj_update_nd_rebuilt")) *value = on ? s->nd_rebuilt : 0;
  else if (!strcmp(key, "bj_band_map_builds")) *value = on ? s->bm_builds : 0;
  else if (!strcmp(key, "bj_band_map_entries")) *value = on && s->d_bm_src ? (double)s->bm_n : 0.0;
  else if (!strcmp(key, "bj_band_map_bytes")) *value = on && s->d_bm_src ? (double)s->bm_bytes : 0.0;
  else if (!strcmp(key, "bj_update_map_s")) *value = on ? s->upd_map_s : 0.0;
  else if (!strcmp(key, "bj_update_copy_s")) *value = on ? s->upd_copy_s : 0.0;
  else if (!strcmp(key, "bj_update_kernel_s")) *value = on ? s->upd_kernel_s : 0.0;
  else if (!strcmp(key, "bj_update_total_s")) *value = on ? s->upd_total_s : 0.0;
  else if (!strcmp(key, "bj_records_address")) *value = on ? (double)(size_t)s->d_Lf : 0.0;
  else if (!strcmp(key, "bj_g4_address")) *value = on ? (double)(size_t)s->d_Lg4 : 0.0;
  else if (!strcmp(key, "bj_coarse_max_dofs")) *value = PA_COARSE_MAX_DOFS;
  else if (!strncmp(key, "bj_coarse_", 10)) {
    const pa_bj_coarse_t* co = &s->co;
    const int con = on && co->on;
    const char* sub = key + 10;
    if (!strcmp(sub, "dofs")) *value = con ? co->nc : 0;
    else if (!strcmp(sub, "vectors")) *value = con ? co->k : 0;
    else if (!strcmp(sub, "aggregates")) *value = con ? co->naggr : 0;
    else if (!strcmp(sub, "chunks")) *value = con ? co->nchunks : 0;
    else if (!strcmp(sub, "bytes")) *value = con ? co->bytes : 0.0;
    else if (!strcmp(sub, "setup_s")) *value = con ? co->setup_s : 0.0;
    else if (!strcmp(sub, "builds")) *value = con ? co->builds : 0;
    else if (!strcmp(sub, "applies")) *value = con ? (double)co->applies : 0.0;
    else if (!strcmp(sub, "einv_address")) *value = con ? (double)(size_t)co->d_Einv : 0.0;
    else return 1;
  }
  else return 1;
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
