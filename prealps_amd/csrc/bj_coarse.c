/*
 * bj_coarse.c -- the coarse space of the two-level block-Jacobi preconditioner, M^-1 = B^-1 + Z E^-1 Z^T:
 * the glue between the preconditioner's state (bj_priv.h), coarse_space.c on the host and coarse.hip on the device.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_priv.h"

#define BJC_FAIL(...) pa_fail_at("preAlps_BlockJacobiSetCoarseSpace", __VA_ARGS__)
#define BJU_FAIL(...) pa_fail_at("preAlps_BlockJacobiUpdateValues", __VA_ARGS__)

void pa_bj_coarse_release(pa_bj_coarse_t* co) {
  pa_rt_free(co->d_zv); pa_rt_free(co->d_ch_row0); pa_rt_free(co->d_ch_nrows); pa_rt_free(co->d_ch_aggr);
  pa_rt_free(co->d_agg_ptr); pa_rt_free(co->d_agg_chunk); pa_rt_free(co->d_Einv); pa_rt_free(co->d_partial);
  pa_rt_free(co->d_c); pa_rt_free(co->d_y);
  free(co->V); free(co->part_aggregate);
  memset(co, 0, sizeof(*co));
}

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
  pa_bj_t* s = pa_bj_state();
  if (s->co.on && pa_rt_sync()) return pa_fail_at(__func__, "%s", pa_rt_error());
  pa_bj_coarse_release(&s->co);
  pa_bj_apply_epoch_bump();
  return 0;
}

/* part_aggregate[p] of the attached coarse space for the np local parts (the caller's, or the default the library
 * chose); *naggr (may be NULL) the number of aggregates */
int preAlps_BlockJacobiGetCoarseAggregates(int* part_aggregate, int* naggr) {
  const pa_bj_t* s = pa_bj_state();
  if (!s->created || !s->co.on) return pa_fail_at(__func__, "no coarse space attached");
  if (!part_aggregate) return pa_fail_at(__func__, " wrong test 'part_aggregate != NULL'");
  memcpy(part_aggregate, s->co.part_aggregate, (size_t)s->np * sizeof(int));
  if (naggr) *naggr = s->co.naggr;
  return 0;
}

int preAlps_BlockJacobiSetCoarseSpace(int k, const double* V, int ldv, const int* part_aggregate, int naggr) {
  pa_bj_t* s = pa_bj_state();
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
  if (!co.V || !co.part_aggregate) { pa_bj_coarse_release(&co); return BJC_FAIL("out of host memory for the %d vectors", k); }
  for (int a = 0; a < k; ++a) memcpy(co.V + (size_t)a * N, V + (size_t)a * ldv, (size_t)N * sizeof(double));
  if (part_aggregate) {
    memcpy(co.part_aggregate, part_aggregate, (size_t)np * sizeof(int));
    co.naggr = naggr;
  } else {
    int* rp = (int*)malloc(((size_t)np + 1) * sizeof(int));
    if (!rp) { pa_bj_coarse_release(&co); return BJC_FAIL("out of host memory"); }
    for (int q = 0; q <= np; ++q) rp[q] = op->rowPos[op->part0 + q] - op->row_off;
    pa_coarse_in_t in = {.m = op->m, .nparts = np, .rowPtr = op->A.rowPtr, .lcol = op->A.colInd, .val = op->A.val,
                         .rowPos = rp, .k = k, .max_dofs = PA_COARSE_MAX_DOFS};
    rc = pa_coarse_default_aggregates(&in, preAlps_hip_partition_kway, co.part_aggregate, &co.naggr, err, sizeof(err));
    free(rp);
    if (rc) { pa_bj_coarse_release(&co); return BJC_FAIL("default aggregates: %s", err[0] ? err : preAlps_hip_last_error()); }
  }
  pa_coarse_t hc;
  rc = bj_coarse_host(s, &co, op, &hc, err, sizeof(err));
  if (rc) { pa_bj_coarse_release(&co); return BJC_FAIL("%s", err); }
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
    pa_bj_coarse_release(&co);
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
  pa_bj_coarse_release(&s->co);     /* setting a coarse space again replaces it (the copies above have drained the stream) */
  s->co = co;
  pa_bj_apply_epoch_bump();
  return 0;
}

/* The coarse space follows the new values and the new scaling vector: zv, E and Einv formed again from the kept V and
 * aggregates and written into the same device arrays (the chunk lists depend on the partition alone).  A singular E
 * drops the coarse space; the block factor is not touched here. */
int pa_bj_coarse_refresh(pa_bj_t* s, const pa_operator_info_t* op) {
  pa_bj_coarse_t* co = &s->co;
  const double t0 = pa_wtime();
  char err[320];
  err[0] = 0;
  pa_coarse_t hc;
  int rc = bj_coarse_host(s, co, op, &hc, err, sizeof(err));
  if (!rc && (hc.nc != co->nc || hc.nchunks != co->nchunks)) { rc = 1; snprintf(err, sizeof(err), "the partition changed"); pa_coarse_free(&hc); }
  if (rc) {
    if (pa_rt_sync()) { /* nothing more to report */ }
    pa_bj_coarse_release(co);
    pa_bj_apply_epoch_bump();
    return BJU_FAIL("the coarse space was dropped, the refreshed block factor stays: %s", err);
  }
  if (pa_rt_h2d(co->d_zv, hc.zv, (size_t)op->m * co->k * sizeof(double)) ||
      pa_rt_h2d(co->d_Einv, hc.Einv, (size_t)hc.nc * hc.nc * sizeof(double))) {
    pa_coarse_free(&hc);
    pa_bj_coarse_release(co);
    pa_bj_apply_epoch_bump();
    return BJU_FAIL("the coarse space was dropped: uploading it failed: %s", pa_rt_error());
  }
  pa_coarse_free(&hc);
  ++co->builds;
  co->setup_s = pa_wtime() - t0;
  return 0;
}
