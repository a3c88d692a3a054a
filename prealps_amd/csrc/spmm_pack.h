/*
 * spmm_pack.h -- the packed form of a run plan's value array (spmm_pack.c).  The run plan (spmm_plan.h) stores
 * three values per run and lane, [slice][step k][position 0..2][lane 0..63]; a caller who assembles whole element
 * matrices hands in many entries that are exactly +0.0, and padding adds more.  The packed form keeps only the
 * values whose bit pattern is not that of +0.0 (a stored -0.0 is kept), densely, in the same order, behind one
 * 0.0 per step, and says per step which lanes hold a value:
 *
 *   meta[4 g + p], p = 0..2   presence mask of position p of step g: bit i set = lane i has a value
 *   meta[4 g + 3]             index b in `val` of the step's part: val[b] = 0.0, the kept values follow
 *   lane i, position p, bit set:    val[b + 1 + (set bits of the masks of positions < p) + (set bits of mask p below i)]
 *   lane i, position p, bit clear:  val[b], the step's own 0.0 (what the kernel reads in place of the dropped +0.0)
 *
 * where g = sl_off[s] / 64 + k counts the steps of all slices in plan order (sl_off is a multiple of 64), so kept
 * value j of step g lies at val[g + 1 + j].  `val` ends in PA_SPMM_PACK_SLACK zeros.  Pure host arithmetic on
 * libc, like spmm_plan.c: it neither reads nor changes the host plan's layout.
 */
#ifndef PA_SPMM_PACK_H
#define PA_SPMM_PACK_H

#include <stddef.h>
#include <stdint.h>

#define PA_SPMM_PACK_SLACK 64

typedef struct {
  uint64_t* meta;        /* 4 * nsteps_alloc entries (the spare step is empty and points at the slack) */
  size_t nsteps, nsteps_alloc;
  double* val;           /* nsteps zeros and nval kept values, then zeros up to nval_alloc */
  size_t nval, nval_alloc;
  uint32_t* pos;         /* pos[j] = index of kept value j in the plan's value array (NULL: not asked for) */
  double packed_bytes;   /* values, step zeros, masks and offsets one product streams */
  double unpacked_bytes; /* the plan's value array */
} pa_spmm_pack_t;

/* Pack the value array `val` (PA_PL_VAL: 192 values per step) of a run plan with the slices sl_off / sl_len
 * (PA_PL_SL_OFF, PA_PL_SL_LEN).  Returns 0; -1 when out of memory; -2 when the plan is too large for 32-bit
 * positions or its slices are not whole steps behind each other.  After a failure `pk` is empty. */
int pa_spmm_pack_build(const double* val, const long long* sl_off, const int* sl_len, int nslices, int want_pos,
                       pa_spmm_pack_t* pk);
/* Release a pack in any state; leaves it empty. */
void pa_spmm_pack_free(pa_spmm_pack_t* pk);

#endif
