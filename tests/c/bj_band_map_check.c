/*
 * bj_band_map_check.c -- the band map behind preAlps_BlockJacobiUpdateValues (prealps_amd/csrc/bj_band_map.c),
 * checked on the host against a direct assembly of every band from the permuted dense diagonal block.  Panels
 * generated here: Poisson 12^3 in 5 contiguous parts, a 3-dof node grid 8^3 in 8 boxes, a random symmetric
 * pattern of 2048 rows in 7 parts, one shard of each grid (global column ids outside the local rows), and the
 * Poisson panel with a row that holds a column twice.  Every block is ordered by the identity, the reversal or
 * a seeded random permutation (the kinds rotate over the blocks, three runs per panel, so one run holds narrow
 * and wide bands: both layouts), with the bandwidth computed from the order; a fourth run flags every third
 * block as sparse-factored.  Per run:
 *   - the band obtained by scattering a value array through the map equals, in bits, the direct assembly, for
 *     two value arrays; a second build gives the same map byte for byte;
 *   - every in-block entry on or below the diagonal (of a doubled column: the last one) is used exactly once,
 *     nothing else is used;
 *   - destinations are unique and inside their block, chunks stay inside a block and within the chunk size;
 *   - flagged blocks contribute nothing.
 * One line per run; a non-zero exit and a line on stderr for every violation.  tests/test_bj_band_map_cpu.py
 * builds it with the host sanitizers.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_band_map.h"

static int g_bad = 0;
#define BAD(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); g_bad = 1; } while (0)

static void* must(void* p) {
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}

typedef struct { int n; int* rp; int* ci; double* v; } csr_t;
static void csr_free(csr_t* A) { free(A->rp); free(A->ci); free(A->v); memset(A, 0, sizeof(*A)); }

static uint64_t g_rng = 88172645463325252ULL;
static uint32_t rnd(void) { g_rng = g_rng * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(g_rng >> 33); }

static double entry(int i, int j) {   /* symmetric, diagonal heavy, no two neighbours alike */
  int lo = i < j ? i : j, hi = i < j ? j : i;
  return i == j ? 30.0 + (i % 5) : -(1.0 + ((lo * 31 + hi * 17) % 7) / 8.0);
}

/* a g^3 grid: box = 0 the 7-point star, 1 the 27-point box; dof unknowns per node, all coupled */
static csr_t grid_matrix(int g, int box, int dof) {
  int n = g * g * g * dof, per = (box ? 27 : 7) * dof, k = 0;
  csr_t A = {n, must(malloc(((size_t)n + 1) * sizeof(int))), must(malloc((size_t)n * per * sizeof(int))),
             must(malloc((size_t)n * per * sizeof(double)))};
  A.rp[0] = 0;
  for (int z = 0; z < g; ++z) for (int y = 0; y < g; ++y) for (int x = 0; x < g; ++x)
    for (int d = 0; d < dof; ++d) {
      int row = ((z * g + y) * g + x) * dof + d;
      for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        if (!box && abs(dx) + abs(dy) + abs(dz) > 1) continue;
        int xx = x + dx, yy = y + dy, zz = z + dz;
        if (xx < 0 || yy < 0 || zz < 0 || xx >= g || yy >= g || zz >= g) continue;
        for (int e = 0; e < dof; ++e) { int col = ((zz * g + yy) * g + xx) * dof + e; A.ci[k] = col; A.v[k] = entry(row, col); ++k; }
      }
      A.rp[row + 1] = k;
    }
  return A;
}

static int cmp_ll(const void* a, const void* b) {
  long long x = *(const long long*)a, y = *(const long long*)b;
  return (x > y) - (x < y);
}
/* diagonal + `draws` random columns per row, mirrored */
static csr_t random_matrix(int n, int draws) {
  size_t cap = (size_t)n * (2 * draws + 1), ne = 0;
  long long* e = must(malloc(cap * sizeof(long long)));
  for (int i = 0; i < n; ++i) {
    e[ne++] = (long long)i * n + i;
    for (int d = 0; d < draws; ++d) { int j = (int)(rnd() % (uint32_t)n); e[ne++] = (long long)i * n + j; e[ne++] = (long long)j * n + i; }
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
  for (int i = 0; i < n; ++i) if (A.rp[i + 1] < A.rp[i]) A.rp[i + 1] = A.rp[i];
  free(e);
  return A;
}

/* B = P A P^T with the rows grouped part by part (original order inside a part); rowPos: nparts + 1 */
static csr_t permute_by_part(const csr_t* A, const int* part, int nparts, int* rowPos) {
  int n = A->n;
  int* newid = must(malloc((size_t)n * sizeof(int)));
  int* old = must(malloc((size_t)n * sizeof(int)));
  memset(rowPos, 0, ((size_t)nparts + 1) * sizeof(int));
  for (int i = 0; i < n; ++i) rowPos[part[i] + 1]++;
  for (int p = 0; p < nparts; ++p) rowPos[p + 1] += rowPos[p];
  int* next = must(malloc((size_t)nparts * sizeof(int)));
  memcpy(next, rowPos, (size_t)nparts * sizeof(int));
  for (int i = 0; i < n; ++i) { newid[i] = next[part[i]]++; old[newid[i]] = i; }
  csr_t B = {n, must(malloc(((size_t)n + 1) * sizeof(int))), must(malloc((size_t)A->rp[n] * sizeof(int))),
             must(malloc((size_t)A->rp[n] * sizeof(double)))};
  int k = 0;
  B.rp[0] = 0;
  for (int r = 0; r < n; ++r) {      /* (the columns of a row stay in the old order: unsorted in the new numbering) */
    for (int e = A->rp[old[r]]; e < A->rp[old[r] + 1]; ++e) { B.ci[k] = newid[A->ci[e]]; B.v[k] = A->v[e]; ++k; }
    B.rp[r + 1] = k;
  }
  free(newid); free(old); free(next);
  return B;
}

/* the row panel of parts [p0, p1): local rows, global column ids */
typedef struct { int np, m; int* rp; int* ci; double* v; int* row0; int* nrows; int* grow0; } panel_t;
static void panel_free(panel_t* P) { free(P->rp); free(P->ci); free(P->v); free(P->row0); free(P->nrows); free(P->grow0); memset(P, 0, sizeof(*P)); }

static panel_t make_panel(const csr_t* B, const int* rowPos, int p0, int p1) {
  panel_t P;
  int lo = rowPos[p0], hi = rowPos[p1], nnz = B->rp[hi] - B->rp[lo];
  P.np = p1 - p0; P.m = hi - lo;
  P.rp = must(malloc(((size_t)P.m + 1) * sizeof(int)));
  P.ci = must(malloc(((size_t)nnz + 2) * sizeof(int)));      /* (+ 2: room for the doubled column) */
  P.v = must(malloc(((size_t)nnz + 2) * sizeof(double)));
  for (int i = 0; i <= P.m; ++i) P.rp[i] = B->rp[lo + i] - B->rp[lo];
  memcpy(P.ci, B->ci + B->rp[lo], (size_t)nnz * sizeof(int));
  memcpy(P.v, B->v + B->rp[lo], (size_t)nnz * sizeof(double));
  P.row0 = must(malloc((size_t)P.np * sizeof(int)));
  P.nrows = must(malloc((size_t)P.np * sizeof(int)));
  P.grow0 = must(malloc((size_t)P.np * sizeof(int)));
  for (int q = 0; q < P.np; ++q) { P.grow0[q] = rowPos[p0 + q]; P.row0[q] = rowPos[p0 + q] - lo; P.nrows[q] = rowPos[p0 + q + 1] - rowPos[p0 + q]; }
  return P;
}

/* row r gets a second entry for the column of its entry at position `at` (a new value), right behind the row's
 * first entry: the later one of the two is the one an assembly that overwrites keeps */
static void double_a_column(panel_t* P, int r, int at) {
  const int nnz = P->rp[P->m], k = P->rp[r] + at, ins = P->rp[r] + 1;
  const int col = P->ci[k];
  memmove(P->ci + ins + 1, P->ci + ins, (size_t)(nnz - ins) * sizeof(int));
  memmove(P->v + ins + 1, P->v + ins, (size_t)(nnz - ins) * sizeof(double));
  P->ci[ins] = col; P->v[ins] = -77.25;
  for (int i = r + 1; i <= P->m; ++i) P->rp[i]++;
}

/* ---- one run -------------------------------------------------------------------------------------- */
static void run(const char* name, const panel_t* P, int shift, int nd_every, int wmax, int chunk) {
  const int np = P->np, nnz = P->rp[P->m];
  char head[200];
  snprintf(head, sizeof(head), "%s shift=%d nd_every=%d wmax=%d chunk=%d", name, shift, nd_every, wmax, chunk);
  int* order = must(malloc((size_t)(P->m ? P->m : 1) * sizeof(int)));
  int* bw = must(calloc((size_t)np, sizeof(int)));
  char* is_nd = must(calloc((size_t)np, 1));
  int bmax = 1;
  for (int q = 0; q < np; ++q) if (P->nrows[q] > bmax) bmax = P->nrows[q];
  int* pos = must(malloc((size_t)bmax * sizeof(int)));
  /* orders and their bandwidths */
  for (int q = 0; q < np; ++q) {
    const int r0 = P->row0[q], b = P->nrows[q], g0 = P->grow0[q], kind = (q + shift) % 3;
    int* o = order + r0;
    for (int j = 0; j < b; ++j) o[j] = kind == 1 ? b - 1 - j : j;
    if (kind == 2) for (int j = b - 1; j > 0; --j) { int x = (int)(rnd() % (uint32_t)(j + 1)), t = o[j]; o[j] = o[x]; o[x] = t; }
    for (int j = 0; j < b; ++j) pos[o[j]] = j;
    for (int i = 0; i < b; ++i)
      for (int k = P->rp[r0 + i]; k < P->rp[r0 + i + 1]; ++k) {
        const int c = P->ci[k];
        if (c < g0 || c >= g0 + b) continue;
        int d = pos[i] - pos[c - g0]; if (d < 0) d = -d; if (d > bw[q]) bw[q] = d;
      }
    is_nd[q] = nd_every > 0 && q % nd_every == 1;
  }
  pa_bj_band_map_in_t in = {.np = np, .rowPtr = P->rp, .colInd = P->ci, .row0 = P->row0, .nrows = P->nrows, .grow0 = P->grow0,
                            .bw = bw, .order = order, .is_nd = is_nd, .wmax = wmax, .chunk = chunk};
  pa_bj_band_map_t M, M2;
  if (pa_bj_band_map_build(&in, &M) || pa_bj_band_map_build(&in, &M2)) { BAD("%s: a build failed", head); goto out; }
  if (M.n != M2.n || M.nchunks != M2.nchunks || memcmp(M.src, M2.src, M.n * 4) || memcmp(M.dst, M2.dst, M.n * 4) ||
      memcmp(M.chunk_blk, M2.chunk_blk, M.nchunks * sizeof(int)) || memcmp(M.chunk_first, M2.chunk_first, (M.nchunks + 1) * 4) ||
      memcmp(M.boff, M2.boff, ((size_t)np + 1) * sizeof(long long)))
    BAD("%s: two builds from the same input differ", head);
  pa_bj_band_map_free(&M2);
  const int cmax = chunk > 0 ? chunk : 1024;
  /* offsets, chunks */
  long long btot = 0;
  for (int q = 0; q < np; ++q) {
    if (M.boff[q] != btot) BAD("%s: boff[%d] = %lld, expected %lld", head, q, M.boff[q], btot);
    if (!is_nd[q]) btot += (long long)P->nrows[q] * (bw[q] + 1);
  }
  if (M.boff[np] != btot) BAD("%s: boff[np] = %lld, expected %lld", head, M.boff[np], btot);
  if (M.n > (size_t)nnz) BAD("%s: %zu entries, the panel has %d", head, M.n, nnz);
  if (M.nchunks && M.chunk_first[0] != 0) BAD("%s: the first chunk starts at %u", head, M.chunk_first[0]);
  if (M.chunk_first[M.nchunks] != M.n) BAD("%s: the chunks end at %u of %zu", head, M.chunk_first[M.nchunks], M.n);
  for (size_t c = 0; c < M.nchunks; ++c) {
    const uint32_t e0 = M.chunk_first[c], e1 = M.chunk_first[c + 1];
    const int q = M.chunk_blk[c];
    if (e1 <= e0 || e1 - e0 > (uint32_t)cmax || e1 > M.n) { BAD("%s: chunk %zu = [%u, %u)", head, c, e0, e1); goto done; }
    if (q < 0 || q >= np || is_nd[q]) { BAD("%s: chunk %zu belongs to block %d", head, c, q); goto done; }
    if (c && M.chunk_blk[c - 1] > q) BAD("%s: chunk %zu goes back to block %d", head, c, q);
    for (uint32_t e = e0; e < e1; ++e) {      /* every source lies in the rows of the chunk's block, ascending */
      if (M.src[e] >= (uint32_t)nnz || (int)M.src[e] < P->rp[P->row0[q]] || (int)M.src[e] >= P->rp[P->row0[q] + P->nrows[q]])
        { BAD("%s: entry %u of block %d reads panel entry %u", head, e, q, M.src[e]); goto done; }
      if (e > e0 && M.src[e] <= M.src[e - 1]) BAD("%s: entry %u does not ascend", head, e);
    }
  }
  {
    /* which entries must be used: in-block, on or below the diagonal, the last one of a doubled column */
    char* want = must(calloc((size_t)nnz + 1, 1));
    int* used = must(calloc((size_t)nnz + 1, sizeof(int)));
    size_t nwant = 0, ndup = 0;
    int rows_blocks = 0, diag_blocks = 0, nnd = 0;
    for (int q = 0; q < np; ++q) {
      const int r0 = P->row0[q], b = P->nrows[q], g0 = P->grow0[q];
      if (is_nd[q]) { ++nnd; continue; }
      if (bw[q] <= wmax) ++rows_blocks; else ++diag_blocks;
      for (int j = 0; j < b; ++j) pos[order[r0 + j]] = j;
      for (int i = 0; i < b; ++i)
        for (int k = P->rp[r0 + i]; k < P->rp[r0 + i + 1]; ++k) {
          const int c = P->ci[k];
          if (c < g0 || c >= g0 + b || pos[c - g0] > pos[i]) continue;
          int later = 0;
          for (int k2 = k + 1; k2 < P->rp[r0 + i + 1]; ++k2) later |= P->ci[k2] == c;
          if (later) ++ndup; else { want[k] = 1; ++nwant; }
        }
    }
    for (size_t e = 0; e < M.n; ++e) ++used[M.src[e]];
    size_t missing = 0, extra = 0, twice = 0;
    for (int k = 0; k < nnz; ++k) { missing += want[k] && !used[k]; extra += !want[k] && used[k]; twice += used[k] > 1; }
    if (missing || extra || twice || nwant != M.n)
      BAD("%s: %zu wanted entries unused, %zu unwanted used, %zu used twice (%zu wanted, %zu in the map)", head, missing, extra, twice, nwant, M.n);
    /* the bands through the map against the direct assembly from the permuted dense block, for two value arrays */
    double* v2 = must(malloc(((size_t)nnz + 1) * sizeof(double)));
    for (int k = 0; k < nnz; ++k) v2[k] = P->v[k] * (0.5 + (double)(((unsigned)k * 2654435761u) >> 20) / 4096.0) + 0.25;
    double* band = must(malloc(((size_t)btot + 1) * sizeof(double)));
    char* hit = must(malloc((size_t)btot + 1));
    double* D = must(malloc((size_t)bmax * bmax * sizeof(double)));
    for (int pass = 0; pass < 2; ++pass) {
      const double* val = pass ? v2 : P->v;
      size_t outside = 0, shared = 0, wrong = 0;
      memset(band, 0, ((size_t)btot + 1) * sizeof(double));
      memset(hit, 0, (size_t)btot + 1);
      for (size_t c = 0; c < M.nchunks; ++c) {
        const int q = M.chunk_blk[c];
        const long long len = (long long)P->nrows[q] * (bw[q] + 1);
        for (uint32_t e = M.chunk_first[c]; e < M.chunk_first[c + 1]; ++e) {
          if ((long long)M.dst[e] >= len) { ++outside; continue; }
          const size_t at = (size_t)(M.boff[q] + M.dst[e]);
          shared += hit[at]; hit[at] = 1;
          band[at] = val[M.src[e]];
        }
      }
      if (outside) BAD("%s: %zu destinations outside their block", head, outside);
      if (shared) BAD("%s: %zu destinations written twice", head, shared);
      for (int q = 0; q < np; ++q) {
        const int r0 = P->row0[q], b = P->nrows[q], g0 = P->grow0[q], w = bw[q];
        if (is_nd[q]) { if (M.boff[q + 1] != M.boff[q]) BAD("%s: sparse block %d has a band", head, q); continue; }
        for (int j = 0; j < b; ++j) pos[order[r0 + j]] = j;
        memset(D, 0, (size_t)b * b * sizeof(double));
        for (int i = 0; i < b; ++i)
          for (int k = P->rp[r0 + i]; k < P->rp[r0 + i + 1]; ++k) {
            const int c = P->ci[k];
            if (c >= g0 && c < g0 + b) D[(size_t)pos[i] * b + pos[c - g0]] = val[k];
          }
        const double* got = band + M.boff[q];
        for (int ni = 0; ni < b; ++ni)
          for (int d = 0; d <= w; ++d) {
            const double ref = ni - d >= 0 ? D[(size_t)ni * b + (ni - d)] : 0.0;
            const double g = w <= wmax ? got[(size_t)ni * (w + 1) + d] : got[(size_t)d * b + ni];
            if (memcmp(&ref, &g, sizeof(double))) ++wrong;
          }
      }
      if (wrong) BAD("%s: %zu band entries differ from the direct assembly (values %d)", head, wrong, pass);
    }
    printf("%s: blocks=%d nd=%d rows=%d diag=%d entries=%zu chunks=%zu doubled=%zu\n", head, np, nnd, rows_blocks, diag_blocks,
           M.n, M.nchunks, ndup);
    free(want); free(used); free(v2); free(band); free(hit); free(D);
  }
done:
  pa_bj_band_map_free(&M);
out:
  free(order); free(bw); free(is_nd); free(pos);
}

static void run_panel(const char* name, const panel_t* P) {
  for (int shift = 0; shift < 3; ++shift) run(name, P, shift, 0, 96, shift == 1 ? 100 : 0);
  run(name, P, 0, 3, 96, 0);
}

int main(void) {
  csr_t poisson = grid_matrix(12, 0, 1), nodes = grid_matrix(8, 1, 3), rndm = random_matrix(2048, 3);
  int rowPos[16];
  int* part = must(malloc((size_t)2048 * sizeof(int)));
  /* Poisson 12^3, 5 contiguous parts */
  for (int i = 0; i < poisson.n; ++i) part[i] = (int)(((long long)i * 5) / poisson.n);
  csr_t B = permute_by_part(&poisson, part, 5, rowPos);
  panel_t P = make_panel(&B, rowPos, 0, 5);
  run_panel("poisson12", &P);
  /* a narrow width limit: the natural order of these blocks (band 144) is row-major under 200 */
  run("poisson12", &P, 0, 0, 200, 0);
  /* a row that holds a column twice: row 200 (block 0), its first in-block entry below the diagonal */
  double_a_column(&P, 200, 0);
  run("poisson12_doubled", &P, 0, 0, 200, 0);
  run("poisson12_doubled", &P, 2, 0, 96, 64);
  panel_free(&P);
  P = make_panel(&B, rowPos, 1, 4);
  run_panel("poisson12_shard", &P);
  panel_free(&P);
  csr_free(&B);
  /* 3 dofs per node, 8^3 nodes, boxes of 4^3 nodes */
  for (int i = 0; i < nodes.n; ++i) {
    const int node = i / 3, x = node % 8, y = (node / 8) % 8, z = node / 64;
    part[i] = (z / 4) * 4 + (y / 4) * 2 + x / 4;
  }
  B = permute_by_part(&nodes, part, 8, rowPos);
  P = make_panel(&B, rowPos, 0, 8);
  run_panel("nodes8", &P);
  panel_free(&P);
  P = make_panel(&B, rowPos, 2, 5);
  run_panel("nodes8_shard", &P);
  panel_free(&P);
  csr_free(&B);
  /* random pattern, 7 contiguous parts */
  for (int i = 0; i < rndm.n; ++i) part[i] = (int)(((long long)i * 7) / rndm.n);
  B = permute_by_part(&rndm, part, 7, rowPos);
  P = make_panel(&B, rowPos, 0, 7);
  run_panel("random2048", &P);
  panel_free(&P);
  csr_free(&B);
  free(part);
  csr_free(&poisson); csr_free(&nodes); csr_free(&rndm);
  return g_bad;
}
