/*
 * spmm_plan_dump.c -- cuts SpMM plans (prealps_amd/csrc/spmm_plan.c) for small generated matrices
 * and prints one line per case: every scalar of the plan and, per array, the elements uploaded, the
 * elements allocated on the device and a 64-bit FNV-1a hash of the uploaded bytes.
 * tests/test_spmm_plan_cpu.py builds it with the host sanitizers and compares the lines with
 * tests/golden/spmm_plan_digests.json.  The cases reach every branch of the plan builders: window,
 * staged and run plans, blocks of several slices and of one, blocks halved until they fit, a slice
 * that overflows the staging area, the 16 -> 8 column split, and shards that read halo rows.
 *
 * With spmm_plan.c compiled -Dmalloc=t_malloc -Dcalloc=t_calloc -Drealloc=t_realloc
 * -Dposix_memalign=t_posix_memalign, `spmm_plan_dump fail-allocs` instead lets the k-th allocation of a build fail, for
 * k = 0, 1, ... until the build succeeds: every failure must be reported, leave an empty plan, and --
 * the sanitizers watch -- neither leak nor touch freed memory.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spmm_plan.h"

static long g_allocs_left = -1;   /* >= 0: that many allocations of spmm_plan.c succeed, the next one fails */
static int alloc_fails(void) { return g_allocs_left >= 0 && g_allocs_left-- == 0; }
void* t_malloc(size_t n) { return alloc_fails() ? NULL : malloc(n); }
void* t_calloc(size_t n, size_t e) { return alloc_fails() ? NULL : calloc(n, e); }
void* t_realloc(void* p, size_t n) { return alloc_fails() ? NULL : realloc(p, n); }
int t_posix_memalign(void** p, size_t a, size_t n) { return alloc_fails() ? 12 : posix_memalign(p, a, n); }

typedef struct { int n; int* rp; int* ci; double* v; } csr_t;

static void* must(void* p) {
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}
static void csr_free(csr_t* A) { free(A->rp); free(A->ci); free(A->v); memset(A, 0, sizeof(*A)); }

static double entry(int i, int j) {   /* symmetric, diagonal heavy */
  int lo = i < j ? i : j, hi = i < j ? j : i;
  return i == j ? 30.0 + (i % 5) : -(1.0 + ((lo * 31 + hi * 17) % 7) / 8.0);
}

/* a g^3 grid: box = 0 the 7-point star, 1 the 27-point box; dof unknowns per node, all coupled */
static csr_t grid_matrix(int g, int box, int dof) {
  int nodes = g * g * g, n = nodes * dof, per = (box ? 27 : 7) * dof;
  csr_t A = {n, must(malloc(((size_t)n + 1) * sizeof(int))), must(malloc((size_t)n * per * sizeof(int))),
             must(malloc((size_t)n * per * sizeof(double)))};
  int k = 0;
  A.rp[0] = 0;
  for (int z = 0; z < g; ++z) for (int y = 0; y < g; ++y) for (int x = 0; x < g; ++x)
    for (int d = 0; d < dof; ++d) {
      int row = ((z * g + y) * g + x) * dof + d;
      for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        if (!box && abs(dx) + abs(dy) + abs(dz) > 1) continue;
        int xx = x + dx, yy = y + dy, zz = z + dz;
        if (xx < 0 || yy < 0 || zz < 0 || xx >= g || yy >= g || zz >= g) continue;
        for (int e = 0; e < dof; ++e) {
          int col = ((zz * g + yy) * g + xx) * dof + e;
          A.ci[k] = col; A.v[k] = entry(row, col); ++k;
        }
      }
      A.rp[row + 1] = k;   /* (dz, dy, dx, e ascending: the columns are sorted) */
    }
  return A;
}

static int cmp_ll(const void* a, const void* b) {
  long long x = *(const long long*)a, y = *(const long long*)b;
  return (x > y) - (x < y);
}
/* diagonal + `draws` random columns per row, mirrored (every row holds its diagonal) */
static csr_t random_matrix(int n, int draws, unsigned seed) {
  size_t cap = (size_t)n * (2 * draws + 1), ne = 0;
  long long* e = must(malloc(cap * sizeof(long long)));
  uint64_t st = seed;
  for (int i = 0; i < n; ++i) {
    e[ne++] = (long long)i * n + i;
    for (int d = 0; d < draws; ++d) {
      st = st * 6364136223846793005ULL + 1442695040888963407ULL;
      int j = (int)((st >> 33) % (uint64_t)n);
      e[ne++] = (long long)i * n + j; e[ne++] = (long long)j * n + i;
    }
  }
  qsort(e, ne, sizeof(long long), cmp_ll);
  csr_t A = {n, must(calloc((size_t)n + 1, sizeof(int))), must(malloc(ne * sizeof(int))), must(malloc(ne * sizeof(double)))};
  int k = 0;
  for (size_t q = 0; q < ne; ++q) {
    if (q && e[q] == e[q - 1]) continue;
    int i = (int)(e[q] / n), j = (int)(e[q] % n);
    A.ci[k] = j; A.v[k] = entry(i, j); ++k;
    A.rp[i + 1] = k;
  }
  free(e);
  return A;
}

/* ---- the panel of subdomains [part0, part1) of nparts contiguous ones -------------------------- */
typedef struct { int m, halo, row_off; int* rowPos; int* rp; int* lcol; double* v; } panel_t;

static void panel_free(panel_t* P) { free(P->rowPos); free(P->rp); free(P->lcol); free(P->v); memset(P, 0, sizeof(*P)); }

/* local column ids as the operator build numbers them: own rows first, then one slot per distinct
 * off-panel column, ascending */
static panel_t make_panel(const csr_t* A, int nparts, int part0, int part1) {
  panel_t P;
  memset(&P, 0, sizeof(P));
  P.rowPos = must(calloc((size_t)nparts + 1, sizeof(int)));
  for (int i = 0; i < A->n; ++i) P.rowPos[(int)(((long long)i * nparts) / A->n) + 1]++;
  for (int p = 0; p < nparts; ++p) P.rowPos[p + 1] += P.rowPos[p];
  int lo = P.rowPos[part0], hi = P.rowPos[part1];
  P.row_off = lo; P.m = hi - lo;
  int nnz = A->rp[hi] - A->rp[lo];
  P.rp = must(malloc(((size_t)P.m + 1) * sizeof(int)));
  P.lcol = must(malloc(((size_t)nnz + 8) * sizeof(int)));
  P.v = must(malloc(((size_t)nnz + 1) * sizeof(double)));
  int* mark = must(calloc((size_t)A->n, sizeof(int)));
  for (int k = A->rp[lo]; k < A->rp[hi]; ++k) { int c = A->ci[k]; if (c < lo || c >= hi) mark[c] = 1; }
  for (int c = 0; c < A->n; ++c) if (mark[c]) mark[c] = ++P.halo;
  for (int i = 0; i <= P.m; ++i) P.rp[i] = A->rp[lo + i] - A->rp[lo];
  for (int k = 0; k < nnz; ++k) {
    int c = A->ci[A->rp[lo] + k];
    P.lcol[k] = (c >= lo && c < hi) ? c - lo : P.m + mark[c] - 1;
    P.v[k] = A->v[A->rp[lo] + k];
  }
  for (int k = nnz; k < nnz + 8; ++k) P.lcol[k] = 0;
  free(mark);
  return P;
}

/* ---- one line per plan ------------------------------------------------------------------------- */
static uint64_t fnv1a(const void* p, size_t bytes) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h = 1469598103934665603ULL;
  for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ULL; }
  return h;
}

static const char* k_names[PA_PL_COUNT] = {"sl_off", "sl_len", "sl_row0", "sl_nrows", "col", "col16", "val",
                                           "blk_slice", "blk_win", "blk_ext_off", "blk_nlow", "ext_rows", "order"};

static int g_failed = 0, g_fail_allocs = 0;

static void fail_allocs(const char* name, const pa_spmm_plan_in_t* in) {
  pa_spmm_host_plan_t pl;
  long k = 0;
  for (;; ++k) {
    g_allocs_left = k;
    int rc = pa_spmm_plan_build(in, &pl);
    int fired = g_allocs_left < 0;
    g_allocs_left = -1;
    if (!fired) { if (rc) g_failed = 1; break; }     /* fewer than k + 1 allocations: the whole build ran */
    int empty = pl.nslices == 0 && pl.nblk == 0;
    for (int i = 0; i < PA_PL_COUNT; ++i) empty = empty && !pl.a[i].p;
    if (rc != -1 || !empty) { printf("%s: failed allocation %ld gave rc=%d, plan %s\n", name, k, rc, empty ? "empty" : "not empty"); g_failed = 1; }
  }
  printf("%s ts=%d cus=%d staged_switch=%d runs_switch=%d: %s, staged=%d runs=%d\n", name, in->ts, in->cus,
         in->want_staged, in->want_runs, k > 8 ? "every failed allocation handled" : "TOO FEW ALLOCATIONS SEEN", pl.staged, pl.runs);
  if (k <= 8) g_failed = 1;
  pa_spmm_plan_free(&pl);
}

static void dump(const char* name, const panel_t* P, int nparts_from, int nparts_to, int ts, int cus, int staged, int runs) {
  pa_spmm_plan_in_t in = {.m = P->m, .halo = P->halo, .part0 = nparts_from, .part1 = nparts_to, .row_off = P->row_off,
                          .rowPos = P->rowPos, .rowPtr = P->rp, .lcol = P->lcol, .val = P->v,
                          .ts = ts, .cus = cus, .want_staged = staged, .want_runs = runs};
  pa_spmm_host_plan_t pl;
  if (g_fail_allocs) { if (cus == 1 && ts <= 8) fail_allocs(name, &in); return; }
  printf("%s ts=%d cus=%d staged_switch=%d runs_switch=%d:", name, ts, cus, staged, runs);
  if (pa_spmm_plan_build(&in, &pl)) { printf(" FAILED\n"); g_failed = 1; return; }
  printf(" m=%d nslices=%d nblk=%d n_interior=%d win_cap=%d staged=%d runs=%d runs_cols=%d stage_cap=%d"
         " sell_entries=%.0f stream_bytes=%.0f",
         pl.m, pl.nslices, pl.nblk, pl.n_interior, pl.win_cap, pl.staged, pl.runs, pl.runs_cols, pl.stage_cap,
         pl.sell_entries, pl.stream_bytes);
  for (int i = 0; i < PA_PL_COUNT; ++i) {
    const pa_plan_array_t* a = &pl.a[i];
    if (!a->p) continue;
    printf(" %s=%zu/%zux%zu:%016llx", k_names[i], a->n, a->n_alloc, a->elem, (unsigned long long)fnv1a(a->p, a->n * a->elem));
  }
  printf("\n");
  pa_spmm_plan_free(&pl);
}

int main(int argc, char** argv) {
  g_fail_allocs = argc > 1 && !strcmp(argv[1], "fail-allocs");
  static const int strides[3] = {4, 8, 16}, cu_counts[2] = {1, 256};
  csr_t poisson = grid_matrix(12, 0, 1);       /* 7-point, 1728 rows */
  csr_t nodes = grid_matrix(8, 1, 3);          /* 27-point, 3 dofs per node, 1536 rows */
  panel_t P = make_panel(&poisson, 5, 0, 5);
  for (int c = 0; c < 2; ++c) for (int t = 0; t < 3; ++t) {
    dump("poisson12", &P, 0, 5, strides[t], cu_counts[c], -1, 1);
    dump("poisson12", &P, 0, 5, strides[t], cu_counts[c], 1, 0);
    dump("poisson12", &P, 0, 5, strides[t], cu_counts[c], 0, 1);
  }
  panel_free(&P);
  P = make_panel(&nodes, 7, 0, 7);
  for (int c = 0; c < 2; ++c) for (int t = 0; t < 3; ++t) {
    dump("nodes8", &P, 0, 7, strides[t], cu_counts[c], -1, 1);
    dump("nodes8", &P, 0, 7, strides[t], cu_counts[c], -1, 0);
  }
  panel_free(&P);
  for (int big = 0; big < 2; ++big) {
    csr_t R = big ? random_matrix(4096, 12, 7u) : random_matrix(2048, 3, 5u);
    P = make_panel(&R, 3, 0, 3);
    for (int t = 0; t < 2; ++t) {
      dump(big ? "random4096" : "random2048", &P, 0, 3, strides[t], 1, 1, 0);
      dump(big ? "random4096" : "random2048", &P, 0, 3, strides[t], 1, -1, 2);
    }
    panel_free(&P);
    csr_free(&R);
  }
  /* middle shards: halo slots behind the own rows, halo-reading blocks last in `order` */
  P = make_panel(&poisson, 5, 1, 4);
  for (int c = 0; c < 2; ++c) for (int t = 0; t < 3; ++t) {
    dump("poisson12_shard", &P, 1, 4, strides[t], cu_counts[c], -1, 1);
    dump("poisson12_shard", &P, 1, 4, strides[t], cu_counts[c], 1, 0);
    dump("poisson12_shard", &P, 1, 4, strides[t], cu_counts[c], 0, 1);
  }
  panel_free(&P);
  P = make_panel(&nodes, 7, 2, 5);
  for (int c = 0; c < 2; ++c) for (int t = 0; t < 3; ++t) {
    dump("nodes8_shard", &P, 2, 5, strides[t], cu_counts[c], -1, 1);
    dump("nodes8_shard", &P, 2, 5, strides[t], cu_counts[c], -1, 0);
    dump("nodes8_shard", &P, 2, 5, strides[t], cu_counts[c], 0, 1);
  }
  panel_free(&P);
  csr_free(&poisson); csr_free(&nodes);
  return g_failed;
}
