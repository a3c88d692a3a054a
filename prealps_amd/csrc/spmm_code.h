/*
 * spmm_code.h -- the packed value array of a run plan (spmm_pack.h) as 2-byte codes into per-block tables
 * (spmm_code.c).  A matrix assembled from one element matrix repeats a handful of bit patterns millions of times;
 * per workgroup block of the plan the distinct patterns of the kept values are few enough to sit in LDS behind the
 * block's staging rows, and the product then streams 2 bytes per value instead of 8:
 *
 *   code[i]                   one per element of pk->val, at the same index (nval_alloc entries): the masks and
 *                             offsets of pk->meta serve both arrays unchanged; a step's own 0.0 and the slack get 0
 *   tab[blk_tab_off[b] + c]   the bits of every element with code c of block b; entry 0 is +0.0, the others are the
 *                             block's distinct patterns, most frequent first, ties by ascending bit pattern
 *
 * Patterns are compared as 64-bit integers: -0.0, NaN payloads and denormals are patterns like any other.  A block
 * is coded iff (nown + next + 2) * ts * 8 + 8 * entries <= budget and entries <= 65536 (its staging rows, the two
 * zero rows and the table within the workgroup's LDS); else it is raw: its table is empty, its codes are 0 and
 * nobody reads them -- the kernels read such a block from the packed fp64 array.  Pure host arithmetic on libc.
 */
#ifndef PA_SPMM_CODE_H
#define PA_SPMM_CODE_H

#include <stddef.h>
#include <stdint.h>

#include "spmm_pack.h"

typedef struct {
  uint16_t* code;        /* ncode entries (= pk->nval_alloc) */
  size_t ncode;
  double* tab;           /* ntab entries (never NULL after a build) */
  size_t ntab;
  int* blk_tab_off;      /* nblk + 1 */
  int nblk, ncoded;      /* blocks, coded blocks */
  size_t coded_elems;    /* elements of pk->val in coded blocks */
  int lds_bytes;         /* staging rows + zero rows + table of the coded block that needs most (0: none coded) */
  double coded_bytes;    /* what one product streams of values, masks and offsets: pk->packed_bytes with 2 bytes
                          * in place of 8 per element of a coded block, and the tables */
} pa_spmm_code_t;

/* Codes and tables for the pack `pk` of a run plan with the blocks blk_slice / blk_ext_off (nblk of them) over the
 * slices sl_off / sl_row0 / sl_nrows, at panel stride ts with `budget` bytes of LDS per workgroup.  Returns 0; -1
 * when out of memory; -2 when the plan is no run plan (runs == 0) or the arrays do not fit each other.  After a
 * failure `cd` is empty. */
int pa_spmm_code_build(const pa_spmm_pack_t* pk, const int* blk_slice, int nblk, const long long* sl_off,
                       const int* sl_row0, const int* sl_nrows, const int* blk_ext_off, int runs, int ts, int budget,
                       pa_spmm_code_t* cd);
/* Release in any state; leaves it empty. */
void pa_spmm_code_free(pa_spmm_code_t* cd);

#endif
