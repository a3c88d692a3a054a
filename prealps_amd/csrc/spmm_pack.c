/*
 * spmm_pack.c -- packs the value array of a run plan: presence masks per step and position, the values that
 * are not +0.0 densely behind each other (spmm_pack.h).  Host arithmetic only.
 */
#include <stdlib.h>
#include <string.h>

#include "spmm_pack.h"

void pa_spmm_pack_free(pa_spmm_pack_t* pk) {
  if (!pk) return;
  free(pk->meta); free(pk->val); free(pk->pos);
  memset(pk, 0, sizeof(*pk));
}

static inline uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}

int pa_spmm_pack_build(const double* val, const long long* sl_off, const int* sl_len, int nslices, int want_pos,
                       pa_spmm_pack_t* pk) {
  memset(pk, 0, sizeof(*pk));
  if (nslices < 0 || !sl_off || (nslices > 0 && (!val || !sl_len))) return -2;
  /* the slices lie behind each other in whole steps of 64 lanes */
  if (sl_off[0] != 0) return -2;
  for (int s = 0; s < nslices; ++s)
    if (sl_len[s] < 0 || sl_off[s + 1] - sl_off[s] != (long long)sl_len[s] * 64) return -2;
  const size_t nsteps = (size_t)(sl_off[nslices] / 64);
  /* (32-bit positions; the kernels address a step's values by 32-bit byte offsets) */
  if (nsteps * 193 + PA_SPMM_PACK_SLACK >= (size_t)UINT32_MAX / 8) return -2;
  const size_t nunpacked = nsteps * 192;
  size_t nval = 0;
  for (size_t i = 0; i < nunpacked; ++i) nval += bits_of(val[i]) != 0;

  pk->nsteps = nsteps;
  pk->nsteps_alloc = nsteps + 1;
  pk->nval = nval;
  pk->nval_alloc = nsteps + nval + PA_SPMM_PACK_SLACK;
  pk->meta = (uint64_t*)malloc(pk->nsteps_alloc * 4 * sizeof(uint64_t));
  pk->val = (double*)malloc(pk->nval_alloc * sizeof(double));
  if (want_pos) pk->pos = (uint32_t*)malloc((nval ? nval : 1) * sizeof(uint32_t));
  if (!pk->meta || !pk->val || (want_pos && !pk->pos)) { pa_spmm_pack_free(pk); return -1; }

  size_t j = 0;   /* kept values so far */
  for (size_t g = 0; g < nsteps; ++g) {
    pk->meta[4 * g + 3] = g + j;
    pk->val[g + j] = 0.0;
    for (int p = 0; p < 3; ++p) {
      const double* v = val + g * 192 + (size_t)p * 64;
      uint64_t mask = 0;
      for (int i = 0; i < 64; ++i) {
        if (bits_of(v[i]) == 0) continue;
        mask |= (uint64_t)1 << i;
        if (pk->pos) pk->pos[j] = (uint32_t)(g * 192 + (size_t)p * 64 + (size_t)i);
        pk->val[g + 1 + j] = v[i];
        ++j;
      }
      pk->meta[4 * g + p] = mask;
    }
  }
  pk->meta[4 * nsteps] = pk->meta[4 * nsteps + 1] = pk->meta[4 * nsteps + 2] = 0;
  pk->meta[4 * nsteps + 3] = nsteps + nval;
  for (size_t i = nsteps + nval; i < pk->nval_alloc; ++i) pk->val[i] = 0.0;
  pk->packed_bytes = (double)(nsteps + nval) * sizeof(double) + (double)nsteps * 4 * sizeof(uint64_t);
  pk->unpacked_bytes = (double)nunpacked * sizeof(double);
  return 0;
}
