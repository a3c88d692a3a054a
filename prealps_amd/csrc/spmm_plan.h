/*
 * spmm_plan.h -- the SpMM plan on the host: local CSR panel in, SELL-64 slices + workgroup blocks
 * out (spmm_plan.c).  Pure host arithmetic on libc: no device call, no environment, no globals, so
 * it runs under a host sanitizer and in tests without a GPU.  operator.c uploads the result.
 */
#ifndef PA_SPMM_PLAN_H
#define PA_SPMM_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "pa_alloc.h"   /* pa_big_alloc */

/* What a plan is cut from; every pointer is borrowed. */
typedef struct {
  int m, halo;           /* own rows, halo slots behind them */
  int part0, part1;      /* subdomains [part0, part1) make up the panel */
  int row_off;           /* global row of local row 0 */
  const int* rowPos;     /* global first row of every subdomain (read at part0 .. part1) */
  const int* rowPtr;     /* m + 1 */
  const int* lcol;       /* local column ids: < m own row, >= m halo slot */
  const double* val;
  int ts;                /* panel stride */
  int cus;               /* compute units of the device (<= 0: 256) */
  int want_staged;       /* PREALPS_SPMM_STAGED: -1 decide, 0 window kernel, 1 force a staged plan */
  int want_runs;         /* PREALPS_SPMM_RUNS: 0 never, 1 when it pays, 2 force */
} pa_spmm_plan_in_t;

/* The arrays of a plan, named after the fields of pa_spmm_plan_t (pa_device.h). */
enum {
  PA_PL_SL_OFF, PA_PL_SL_LEN, PA_PL_SL_ROW0, PA_PL_SL_NROWS, PA_PL_COL, PA_PL_COL16, PA_PL_VAL,
  PA_PL_BLK_SLICE, PA_PL_BLK_WIN, PA_PL_BLK_EXT_OFF, PA_PL_BLK_NLOW, PA_PL_EXT_ROWS, PA_PL_ORDER,
  PA_PL_COUNT
};
typedef struct {
  void* p;          /* NULL: the plan has no such array */
  size_t elem;      /* bytes per element */
  size_t n;         /* elements the kernels are given (the upload copies these) */
  size_t n_alloc;   /* elements of the device array (>= n: never empty, spare entries the kernels read) */
} pa_plan_array_t;

/* A plan on the host; owns its arrays. */
typedef struct {
  int m, nslices, nblk, n_interior;
  int win_cap;                    /* window plan: rows of the largest window */
  int staged, runs, runs_cols, stage_cap;
  double sell_entries;            /* stored entries including padding */
  double stream_bytes;            /* bytes of matrix data one SpMM streams */
  size_t oom_entries;             /* after a failure: the SELL entries the window plan had no memory for (else 0) */
  pa_plan_array_t a[PA_PL_COUNT];
} pa_spmm_host_plan_t;

/* The plan for `in`: the run plan, else the staged plan, else the window plan, each where it is
 * allowed, fits and pays.  Returns 0, or -1 when out of memory (the plan is then empty). */
int pa_spmm_plan_build(const pa_spmm_plan_in_t* in, pa_spmm_host_plan_t* pl);
/* Release a plan in any state (also half built); leaves it empty. */
void pa_spmm_plan_free(pa_spmm_host_plan_t* pl);

/* Where the values of a plan come from.  No decision of a builder reads a value, so the `val` array of the
 * plan for `in` is a fixed gather of the panel's values: val[s] = map[s] ? in->val[map[s] - 1] : 0.0 for the
 * n slots the upload copies (0: padding).  The map is read off a second pa_spmm_plan_build with the same
 * input and the values k + 1 (exact in a double for every int32 count) in place of in->val, which is not
 * read: the builders stay as they are and the map cannot drift from them.  The scalars are those of that
 * second plan, for the caller to hold against the plan it has. */
typedef struct {
  uint32_t* map;   /* n entries; release with free() */
  size_t n;        /* = a[PA_PL_VAL].n of the plan */
  int nslices, nblk, staged, runs, runs_cols;
} pa_spmm_value_map_t;
/* Returns 0, or -1 when out of memory (vm->map is then NULL). */
int pa_spmm_plan_value_map(const pa_spmm_plan_in_t* in, pa_spmm_value_map_t* vm);

#endif
