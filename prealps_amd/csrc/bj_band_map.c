/*
 * bj_band_map.c -- the band map of the block-Jacobi preconditioner (bj_band_map.h): which panel entry every
 * entry of the assembled bands is.  The order of a block, its bandwidth and the layout of its band depend on
 * the pattern alone, so new values for the same pattern reach the bands through a fixed scatter, and the
 * numeric refactorisation (preAlps_BlockJacobiUpdateValues) needs no host assembly.
 */
#include <stdlib.h>
#include <string.h>

#include "bj_band_map.h"

/* The entries of block q in panel order; pos / mark: scratch of nrows[q] ints, pos filled here.  src == NULL:
 * count only.  (size_t)-1: an entry lies outside the band. */
static size_t block_entries(const pa_bj_band_map_in_t* in, int q, int* pos, int* mark, uint32_t* src, uint32_t* dst) {
  const int r0 = in->row0[q], b = in->nrows[q], w = in->bw[q];
  const int g0 = in->grow0[q], g1 = g0 + b;
  const int rows = w <= in->wmax;
  size_t n = 0;
  for (int j = 0; j < b; ++j) pos[in->order[r0 + j]] = j;
  for (int i = 0; i < b; ++i) mark[i] = -1;
  for (int i = 0; i < b; ++i) {
    const int ni = pos[i];
    const int k0 = in->rowPtr[r0 + i], k1 = in->rowPtr[r0 + i + 1];
    /* a column that the row holds twice: the last entry is the one an assembly that overwrites keeps */
    for (int k = k0; k < k1; ++k) { const int c = in->colInd[k]; if (c >= g0 && c < g1) mark[c - g0] = k; }
    for (int k = k0; k < k1; ++k) {
      const int c = in->colInd[k];
      if (c < g0 || c >= g1 || mark[c - g0] != k) continue;
      const int nj = pos[c - g0];
      if (nj > ni) continue;
      if (ni - nj > w) return (size_t)-1;     /* bw is not the bandwidth of this order */
      if (src) {
        src[n] = (uint32_t)k;
        dst[n] = rows ? (uint32_t)((size_t)ni * ((size_t)w + 1) + (size_t)(ni - nj))
                      : (uint32_t)((size_t)(ni - nj) * (size_t)b + (size_t)ni);
      }
      ++n;
    }
  }
  return n;
}

void pa_bj_band_map_free(pa_bj_band_map_t* map) {
  free(map->src); free(map->dst); free(map->chunk_blk); free(map->chunk_first); free(map->boff);
  memset(map, 0, sizeof(*map));
}

int pa_bj_band_map_build(const pa_bj_band_map_in_t* in, pa_bj_band_map_t* map) {
  const int np = in->np;
  const size_t chunk = in->chunk > 0 ? (size_t)in->chunk : 1024;
  memset(map, 0, sizeof(*map));
  map->bad_block = -1;
  int bmax = 1;
  size_t* first = (size_t*)calloc((size_t)np + 1, sizeof(size_t));     /* first entry of every block */
  size_t* cfirst = (size_t*)calloc((size_t)np + 1, sizeof(size_t));    /* first chunk of every block */
  map->boff = (long long*)calloc((size_t)np + 1, sizeof(long long));
  int rc = (!first || !cfirst || !map->boff) ? -1 : 0;
  long long btot = 0;
  for (int q = 0; q < np && !rc; ++q) {
    map->boff[q] = btot;
    if (in->is_nd[q]) continue;
    const long long len = pa_bj_band_len(in->nrows[q], in->bw[q], 0);
    if (len >= (1LL << 32)) { map->bad_block = q; rc = -2; break; }
    btot += len;
    if (in->nrows[q] > bmax) bmax = in->nrows[q];
  }
  if (!rc) map->boff[np] = btot;
  int* pos = NULL; int* mark = NULL;
  if (!rc) {
    pos = (int*)malloc((size_t)bmax * sizeof(int));
    mark = (int*)malloc((size_t)bmax * sizeof(int));
    if (!pos || !mark) rc = -1;
  }
  /* pass 1: count */
  for (int q = 0; q < np && !rc; ++q) {
    const size_t n = in->is_nd[q] ? 0 : block_entries(in, q, pos, mark, NULL, NULL);
    if (n == (size_t)-1) { map->bad_block = q; rc = -3; break; }
    first[q + 1] = first[q] + n;
    cfirst[q + 1] = cfirst[q] + (n + chunk - 1) / chunk;
  }
  if (!rc && first[np] >= ((size_t)1 << 32)) rc = -1;   /* (a panel has fewer entries than 2^31) */
  if (!rc) {
    map->n = first[np]; map->nchunks = cfirst[np];
    map->src = (uint32_t*)malloc((map->n ? map->n : 1) * sizeof(uint32_t));
    map->dst = (uint32_t*)malloc((map->n ? map->n : 1) * sizeof(uint32_t));
    map->chunk_blk = (int*)malloc((map->nchunks ? map->nchunks : 1) * sizeof(int));
    map->chunk_first = (uint32_t*)malloc((map->nchunks + 1) * sizeof(uint32_t));
    if (!map->src || !map->dst || !map->chunk_blk || !map->chunk_first) rc = -1;
  }
  /* pass 2: fill, and cut every block's entries into chunks */
  for (int q = 0; q < np && !rc; ++q) {
    if (in->is_nd[q]) continue;
    (void)block_entries(in, q, pos, mark, map->src + first[q], map->dst + first[q]);
    size_t c = cfirst[q];
    for (size_t e = first[q]; e < first[q + 1]; e += chunk, ++c) { map->chunk_blk[c] = q; map->chunk_first[c] = (uint32_t)e; }
  }
  if (!rc) map->chunk_first[map->nchunks] = (uint32_t)map->n;
  free(pos); free(mark); free(first); free(cfirst);
  if (rc) { const int bad = map->bad_block; pa_bj_band_map_free(map); map->bad_block = bad; }
  return rc;
}
