/* Stand-alone driver of prealps_amd/csrc/coarse_space.c for tests/test_coarse_ranks_cpu.py: the two stages of the build
 * as several processes run them.  Reads one case, cuts the rows after whole parts into "ranks", runs stage (a)
 * (pa_coarse_share) per rank on that rank's rows alone, adds the E_r in rank order, runs stage (b) (pa_coarse_invert),
 * and writes that beside what pa_coarse_build makes of the whole matrix.
 *
 *   coarse_ranks_check IN OUT
 * IN:  8 ints  N, nparts, k, naggr (0: default aggregates, rank by rank), max_dofs (0: the unit's cap), threads, nnz, R
 *      rowPtr[N + 1], col[nnz] (ints), val[nnz] (doubles), rowPos[nparts + 1], part_aggregate[nparts] (ints; read only
 *      when naggr > 0), Vp[N * k] (doubles, row major), cut[R + 1] (ints: rank r owns the parts cut[r] .. cut[r + 1] - 1)
 * OUT: int rc (0, or 100 * (rank + 1) + the code's magnitude for a stage (a) refusal, 1000 + for stage (b), 2000 + for
 *      pa_coarse_build, 3000 + for the default aggregates); 256 bytes of message; ints nc, naggr; part_aggregate[nparts];
 *      R ints: aggregates per rank (default aggregates; otherwise zeros); and when rc = 0:
 *      per rank: ints m, nchunks, nrows; ch_row0, ch_nrows, ch_aggr [nchunks]; agg_ptr [naggr + 1]; agg_chunk [nchunks];
 *                rows [nrows]; zv [m * k]
 *      then doubles, nc * nc each: E and Einv of the ranks, E and Einv of pa_coarse_build, Eabs(x, y) = sum |zv_i[a]
 *      a_ij Vp_j[b]| over the terms of entry (x, y), and terms(x, y), their number.
 * The partitioner handed to the default aggregation cuts the nodes into contiguous ranges, as coarse_space_check.c's. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "coarse_space.h"

static int ranges_kway(int n, const int* rowPtr, const int* colInd, int nparts, int* part) {
  for (int i = 0; i < n; ++i) {          /* the graph must be what the unit promises: sorted rows with a diagonal */
    int diag = 0;
    for (int e = rowPtr[i]; e < rowPtr[i + 1]; ++e) {
      if (colInd[e] == i) diag = 1;
      if (colInd[e] < 0 || colInd[e] >= n || (e > rowPtr[i] && colInd[e] <= colInd[e - 1])) return 1;
    }
    if (!diag) return 1;
  }
  for (int i = 0; i < n; ++i) part[i] = (int)((long long)i * nparts / n);
  return 0;
}

static void* rd(FILE* f, size_t n, size_t elem) {
  void* p = malloc(n * elem + 1);
  if (!p || fread(p, elem, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int h[8];
  if (fread(h, sizeof(int), 8, f) != 8) { fprintf(stderr, "short input\n"); return 2; }
  const int N = h[0], np = h[1], k = h[2], nnz = h[6], R = h[7];
  int naggr = h[3];
  int* rowPtr = (int*)rd(f, (size_t)N + 1, sizeof(int));
  int* col = (int*)rd(f, (size_t)nnz, sizeof(int));
  double* val = (double*)rd(f, (size_t)nnz, sizeof(double));
  int* rowPos = (int*)rd(f, (size_t)np + 1, sizeof(int));
  int* pa = naggr > 0 ? (int*)rd(f, (size_t)np, sizeof(int)) : (int*)calloc((size_t)np, sizeof(int));
  double* Vp = (double*)rd(f, (size_t)N * k, sizeof(double));
  int* cut = (int*)rd(f, (size_t)R + 1, sizeof(int));
  fclose(f);

  char msg[256];
  memset(msg, 0, sizeof(msg));
  int rc = 0;
  int* per_rank = (int*)calloc((size_t)R, sizeof(int));
  int** lrp = (int**)calloc((size_t)R, sizeof(int*));           /* every rank's own row pointer, counted from 0 */
  pa_coarse_share_in_t* in = (pa_coarse_share_in_t*)calloc((size_t)R, sizeof(*in));
  pa_coarse_t* sh = (pa_coarse_t*)calloc((size_t)R, sizeof(*sh));
  for (int r = 0; r < R; ++r) {
    const int r0 = rowPos[cut[r]], m = rowPos[cut[r + 1]] - r0, e0 = rowPtr[r0];
    lrp[r] = (int*)malloc(((size_t)m + 1) * sizeof(int));
    for (int i = 0; i <= m; ++i) lrp[r][i] = rowPtr[r0 + i] - e0;
    in[r] = (pa_coarse_share_in_t){.m = m, .row_off = r0, .nparts = np, .part0 = cut[r], .np_loc = cut[r + 1] - cut[r],
                                   .rowPtr = lrp[r], .gcol = col + e0, .val = val + e0, .rowPos = rowPos, .part_aggregate = pa,
                                   .k = k, .Vp = Vp, .max_dofs = h[4], .threads = h[5]};
  }
  if (naggr <= 0) {        /* the default aggregates: every rank its own parts, numbered rank after rank */
    naggr = 0;
    for (int r = 0; r < R && !rc; ++r) {
      int n = 0;
      int* loc = (int*)malloc(((size_t)in[r].np_loc + 1) * sizeof(int));
      rc = pa_coarse_default_aggregates_share(&in[r], ranges_kway, loc, &n, msg, sizeof(msg));
      if (rc) rc = 3000 - rc;
      for (int q = 0; q < in[r].np_loc && !rc; ++q) pa[cut[r] + q] = naggr + loc[q];
      per_rank[r] = n;
      naggr += n;
      free(loc);
    }
  }
  const int nc = naggr * k;
  const size_t nn = (size_t)nc * nc;
  pa_coarse_t all, whole;
  memset(&all, 0, sizeof(all));
  memset(&whole, 0, sizeof(whole));
  for (int r = 0; r < R && !rc; ++r) {
    in[r].naggr = naggr;
    rc = pa_coarse_share(&in[r], &sh[r], msg, sizeof(msg));
    if (rc) rc = 100 * (r + 1) - rc;
  }
  double* Esum = (double*)calloc(nn ? nn : 1, sizeof(double));
  double* Einv = (double*)calloc(nn ? nn : 1, sizeof(double));
  double* Eabs = (double*)calloc(nn ? nn : 1, sizeof(double));
  double* terms = (double*)calloc(nn ? nn : 1, sizeof(double));
  if (!rc) {
    /* what the all-reduce does: the shares added in rank order */
    memcpy(Esum, sh[0].E, nn * sizeof(double));
    for (int r = 1; r < R; ++r) for (size_t x = 0; x < nn; ++x) Esum[x] += sh[r].E[x];
    /* stage (b) on the sum, in a space of its own (the shares are written out below) */
    all.k = k; all.naggr = naggr; all.nc = nc;
    all.E = (double*)malloc((nn ? nn : 1) * sizeof(double));
    all.Einv = (double*)malloc((nn ? nn : 1) * sizeof(double));
    memcpy(all.E, Esum, nn * sizeof(double));
    rc = pa_coarse_invert(&all, h[5], msg, sizeof(msg));
    if (rc) rc = 1000 - rc;
    else memcpy(Einv, all.Einv, nn * sizeof(double));
  }
  if (!rc) {
    int* rp0 = (int*)malloc(((size_t)np + 1) * sizeof(int));
    memcpy(rp0, rowPos, ((size_t)np + 1) * sizeof(int));
    pa_coarse_in_t win = {.m = N, .nparts = np, .rowPtr = rowPtr, .lcol = col, .val = val, .rowPos = rp0, .part_aggregate = pa,
                          .naggr = naggr, .k = k, .Vp = Vp, .max_dofs = h[4], .threads = h[5]};
    rc = pa_coarse_build(&win, &whole, msg, sizeof(msg));
    if (rc) rc = 2000 - rc;
    free(rp0);
  }
  if (!rc) {        /* the magnitude of every entry's sum and the number of its terms */
    int* row_aggr = (int*)malloc(((size_t)N + 1) * sizeof(int));
    for (int p = 0; p < np; ++p) for (int i = rowPos[p]; i < rowPos[p + 1]; ++i) row_aggr[i] = pa[p];
    for (int i = 0; i < N; ++i)
      for (int e = rowPtr[i]; e < rowPtr[i + 1]; ++e) {
        const int j = col[e], g = row_aggr[i], hh = row_aggr[j];
        for (int a = 0; a < k; ++a)
          for (int b = 0; b < k; ++b) {
            const size_t x = ((size_t)g * k + a) * nc + (size_t)hh * k + b;
            Eabs[x] += fabs(Vp[(size_t)i * k + a] * val[e] * Vp[(size_t)j * k + b]);
            terms[x] += 1.0;
          }
      }
    free(row_aggr);
  }
  printf("rc %d nc %d ranks %d\n", rc, nc, R);

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  int oh[2] = {nc, naggr};
  fwrite(&rc, sizeof(int), 1, o); fwrite(msg, 1, sizeof(msg), o); fwrite(oh, sizeof(int), 2, o);
  fwrite(pa, sizeof(int), (size_t)np, o); fwrite(per_rank, sizeof(int), (size_t)R, o);
  if (!rc) {
    for (int r = 0; r < R; ++r) {
      const pa_coarse_t* c = &sh[r];
      int rh[3] = {c->m, c->nchunks, c->nrows};
      fwrite(rh, sizeof(int), 3, o);
      fwrite(c->ch_row0, sizeof(int), (size_t)c->nchunks, o); fwrite(c->ch_nrows, sizeof(int), (size_t)c->nchunks, o);
      fwrite(c->ch_aggr, sizeof(int), (size_t)c->nchunks, o); fwrite(c->agg_ptr, sizeof(int), (size_t)naggr + 1, o);
      fwrite(c->agg_chunk, sizeof(int), (size_t)c->nchunks, o); fwrite(c->rows, sizeof(int), (size_t)c->nrows, o);
      fwrite(c->zv, sizeof(double), (size_t)c->m * k, o);
    }
    fwrite(Esum, sizeof(double), nn, o); fwrite(Einv, sizeof(double), nn, o);
    fwrite(whole.E, sizeof(double), nn, o); fwrite(whole.Einv, sizeof(double), nn, o);
    fwrite(Eabs, sizeof(double), nn, o); fwrite(terms, sizeof(double), nn, o);
  }
  fclose(o);
  for (int r = 0; r < R; ++r) { pa_coarse_free(&sh[r]); free(lrp[r]); }
  pa_coarse_free(&all); pa_coarse_free(&whole);
  free(Esum); free(Einv); free(Eabs); free(terms); free(per_rank); free(lrp); free(in); free(sh);
  free(rowPtr); free(col); free(val); free(rowPos); free(pa); free(Vp); free(cut);
  return 0;
}
