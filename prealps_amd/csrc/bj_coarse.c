/*
 * bj_coarse.c -- the coarse space of the two-level block-Jacobi preconditioner, M^-1 = B^-1 + Z E^-1 Z^T:
 * the glue between the preconditioner's state (bj_priv.h), coarse_space.c on the host and coarse.hip on the device.
 *
 * Several processes: the attach and the refresh are collective.  Every rank passes the same global V and aggregates and
 * runs stage (a) of coarse_space.h on its own rows; the shares E_r are summed by pa_allreduce on a device buffer and
 * every rank runs stage (b) on the same bits, so a singular E is refused everywhere without a further message.  What
 * one rank alone can find wrong (its copy of V, memory, an upload) is agreed on before any rank returns
 * (pa_ranks_agree): the ranks not at fault report that another process refused, and nobody has changed anything yet.
 * The device keeps the rows of the inverse that the rank's own aggregates need.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_priv.h"

#define BJC_FAIL(...) pa_fail_at("preAlps_BlockJacobiSetCoarseSpace", __VA_ARGS__)
#define BJU_FAIL(...) pa_fail_at("preAlps_BlockJacobiUpdateValues", __VA_ARGS__)
#define BJC_OTHER "another process refused the coarse space"

/* the rehearsal of one shard has nobody to ask (and is refused) */
static int bjc_multi(void) { return pa_world_size() > 1 && !pa_comm_is_loopback(); }

void pa_bj_coarse_release(pa_bj_coarse_t* co) {
  pa_rt_free(co->d_zv); pa_rt_free(co->d_ch_row0); pa_rt_free(co->d_ch_nrows); pa_rt_free(co->d_ch_aggr);
  pa_rt_free(co->d_agg_ptr); pa_rt_free(co->d_agg_chunk); pa_rt_free(co->d_Einv); pa_rt_free(co->d_partial);
  pa_rt_free(co->d_c); pa_rt_free(co->d_y); pa_rt_free(co->d_rows);
  free(co->V); free(co->part_aggregate);
  memset(co, 0, sizeof(*co));
}

/* Stage (a) on this process's rows: zv, the chunk lists, the row list and E_r on the host from the vectors and
 * aggregates in `co` and the operator's current panel, permutation and scaling.  Vp = (D^-1 V)[perm] is formed for the
 * local rows and, on several processes, for the halo columns the panel touches.  The reason of a failure goes to err. */
static int bj_coarse_share(const pa_bj_t* s, const pa_bj_coarse_t* co, const pa_operator_info_t* op, pa_coarse_t* hc,
                           char* err, size_t errlen) {
  const int m = op->m, k = co->k, N = op->N, off = op->row_off, multi = bjc_multi();
  double* Vp = (double*)malloc(((size_t)N * k + 1) * sizeof(double));
  char* touched = multi ? (char*)calloc((size_t)N + 1, 1) : NULL;
  if (!Vp || (multi && !touched)) { free(Vp); free(touched); snprintf(err, errlen, "out of host memory"); return PA_COARSE_NOMEM; }
  if (multi) {
    const int* ci = op->A.colInd;
    const int nnz = op->A.rowPtr[m];
    for (int e = 0; e < nnz; ++e) if (ci[e] >= 0 && ci[e] < N) touched[ci[e]] = 1;
  }
#pragma omp parallel for num_threads(pa_host_threads()) schedule(static)
  for (int g = 0; g < N; ++g) {
    if (!((g >= off && g - off < m) || (touched && touched[g]))) continue;
    const int old = op->perm[g];
    const double d = op->scaling ? op->scaling[old] : 1.0;
    for (int a = 0; a < k; ++a) Vp[(size_t)g * k + a] = co->V[(size_t)a * co->n + old] / d;
  }
  pa_coarse_share_in_t in = {.m = m, .row_off = off, .nparts = op->nparts, .part0 = op->part0, .np_loc = s->np,
                             .rowPtr = op->A.rowPtr, .gcol = op->A.colInd, .val = op->A.val, .rowPos = op->rowPos,
                             .part_aggregate = co->part_aggregate, .naggr = co->naggr, .k = k, .Vp = Vp,
                             .max_dofs = PA_COARSE_MAX_DOFS, .threads = pa_host_threads()};
  const int rc = pa_coarse_share(&in, hc, err, errlen);
  free(Vp); free(touched);
  return rc;
}

/* Stages (a) and (b).  rc: what this process has found wrong so far (its reason in err); on several processes it still
 * takes part in the collectives.  One process: the arithmetic of pa_coarse_build.  Several: the E_r are summed on the
 * device between the stages; a failure before the sum is agreed on here (*settled = 1: every process returns nonzero),
 * one after it -- the download, or the singular E that every process finds alike -- is left to the caller's own
 * agreement.  Nonzero: *hc is empty. */
static int bj_coarse_form(const pa_bj_t* s, const pa_bj_coarse_t* co, const pa_operator_info_t* op, pa_coarse_t* hc, int rc,
                          int* settled, char* err, size_t errlen) {
  *settled = 0;
  memset(hc, 0, sizeof(*hc));
  if (!rc) rc = bj_coarse_share(s, co, op, hc, err, errlen);
  if (!bjc_multi()) {
    *settled = 1;
    return rc ? rc : pa_coarse_invert(hc, pa_host_threads(), err, errlen);
  }
  const size_t nn = rc ? 0 : (size_t)hc->nc * hc->nc;
  double* dE = NULL;
  if (!rc) {
    dE = (double*)pa_rt_malloc(nn * sizeof(double));
    if (!dE || pa_rt_h2d(dE, hc->E, nn * sizeof(double))) {
      rc = 1;
      snprintf(err, errlen, "staging the %d x %d coarse matrix on the device failed: %s", hc->nc, hc->nc, pa_rt_error());
    }
  }
  if (pa_ranks_agree(rc != 0, NULL)) {
    if (!rc) { rc = 1; snprintf(err, errlen, BJC_OTHER); }
    pa_rt_free(dE);
    pa_coarse_free(hc);
    *settled = 1;
    return rc;
  }
  if (pa_allreduce(dE, (int)nn) || pa_rt_d2h(hc->E, dE, nn * sizeof(double))) {
    rc = 1;
    snprintf(err, errlen, "summing the coarse matrix over the processes failed: %s", pa_rt_error());
  }
  pa_rt_free(dE);
  if (rc) pa_coarse_free(hc);
  else rc = pa_coarse_invert(hc, pa_host_threads(), err, errlen);
  return rc;
}

/* zv and the inverse -- on several processes the listed rows of it -- into the device arrays of `co` */
static int bj_coarse_upload(const pa_bj_coarse_t* co, const pa_coarse_t* hc) {
  const size_t nc = (size_t)hc->nc;
  if (pa_rt_h2d(co->d_zv, hc->zv, (size_t)hc->m * hc->k * sizeof(double))) return 1;
  if (!co->multi) return pa_rt_h2d(co->d_Einv, hc->Einv, nc * nc * sizeof(double));
  /* the rows of an aggregate are consecutive: k rows at a time */
  for (int x = 0; x < hc->nrows; x += hc->k)
    if (pa_rt_h2d(co->d_Einv + (size_t)x * nc, hc->Einv + (size_t)hc->rows[x] * nc, (size_t)hc->k * nc * sizeof(double))) return 1;
  return 0;
}

int preAlps_BlockJacobiClearCoarseSpace(void) {
  pa_bj_t* s = pa_bj_state();
  if (s->co.on && pa_rt_sync()) return pa_fail_at(__func__, "%s", pa_rt_error());
  pa_bj_coarse_release(&s->co);
  pa_bj_apply_epoch_bump();
  return 0;
}

/* part_aggregate[p] of the attached coarse space for the operator's nparts parts -- on several processes the parts of
 * all of them -- (the caller's, or the default the library chose); *naggr (may be NULL) the number of aggregates */
int preAlps_BlockJacobiGetCoarseAggregates(int* part_aggregate, int* naggr) {
  const pa_bj_t* s = pa_bj_state();
  if (!s->created || !s->co.on) return pa_fail_at(__func__, "no coarse space attached");
  if (!part_aggregate) return pa_fail_at(__func__, " wrong test 'part_aggregate != NULL'");
  memcpy(part_aggregate, s->co.part_aggregate, (size_t)s->co.nparts * sizeof(int));
  if (naggr) *naggr = s->co.naggr;
  return 0;
}

/* What this process can find wrong with the call by itself, in the order of the one-process refusals; the reason in err. */
static int bjc_args(const pa_bj_t* s, const pa_operator_info_t* op, int k, const double* V, int ldv, const int* part_aggregate,
                    int naggr, char* err, size_t errlen) {
#define BJC_NO(...) do { snprintf(err, errlen, __VA_ARGS__); return 1; } while (0)
  if (k < 1 || k > PA_COARSE_MAX_VECS) BJC_NO("k = %d vectors refused: 1 .. %d", k, PA_COARSE_MAX_VECS);
  if (!V) BJC_NO(" wrong test 'V != NULL'");
  const int N = op->N;
  if (ldv < N) BJC_NO("ldv = %d is smaller than the %d rows of the matrix", ldv, N);
  for (int a = 0; a < k; ++a)
    for (int i = 0; i < N; ++i)
      if (!isfinite(V[(size_t)a * ldv + i])) BJC_NO("V(%d, %d) is not finite", i, a);
  if (part_aggregate && (long long)naggr * k > PA_COARSE_MAX_DOFS)
    BJC_NO("%d aggregates x %d vectors = %lld coarse unknowns, the cap is %d", naggr, k, (long long)naggr * k, PA_COARSE_MAX_DOFS);
  if (part_aggregate && naggr < 1) BJC_NO("naggr = %d refused", naggr);
  if (pa_operator_plan_only()) BJC_NO("the operator was built in plan-only mode (no GPU)");
  if (pa_comm_is_loopback())
    BJC_NO("a preAlps_hip_loopback shard holds the rows of one rank of %d: the coarse matrix needs the rows of all of them",
           pa_world_size());
  if (!s->created) BJC_NO("preconditioner not created");
  if (pa_operator_build_count() != s->op_build || s->A_rowptr != op->A.rowPtr)
    BJC_NO("the preconditioner was not created from the current operator's own panel");
  return 0;
#undef BJC_NO
}

/* The default aggregates on several processes: every rank cuts its own parts (pa_coarse_default_aggregates_share), then
 * one all-reduce on a small device buffer of doubles assembles the global vector -- three slots per rank (its aggregates,
 * its parts, 1 if it failed) and one per part, each filled by its owner alone, so the sums are exact integers.  The
 * aggregates are numbered rank after rank.  Collective: a process whose own step failed (rc, err) still takes part.
 * Nonzero and *settled = 1: every process returns nonzero. */
static int bjc_default_ranks(const pa_bj_t* s, const pa_operator_info_t* op, pa_bj_coarse_t* co, int rc, int* settled,
                             char* err, size_t errlen) {
  const int W = pa_world_size(), me = pa_world_rank(), npg = op->nparts, npl = s->np, cnt = 3 * W + npg;
  *settled = 0;
  int nloc = 0;
  int* loc = (int*)malloc((size_t)(npl ? npl : 1) * sizeof(int));
  double* h = (double*)calloc((size_t)cnt, sizeof(double));
  if (!rc && (!loc || !h)) { rc = 1; snprintf(err, errlen, "out of host memory"); }
  if (!rc) {
    pa_coarse_share_in_t in = {.m = op->m, .row_off = op->row_off, .nparts = npg, .part0 = op->part0, .np_loc = npl,
                               .rowPtr = op->A.rowPtr, .gcol = op->A.colInd, .val = op->A.val, .rowPos = op->rowPos,
                               .k = co->k, .max_dofs = PA_COARSE_MAX_DOFS};
    char why[256];
    why[0] = 0;
    if (pa_coarse_default_aggregates_share(&in, preAlps_hip_partition_kway, loc, &nloc, why, sizeof(why))) {
      rc = 1;
      snprintf(err, errlen, "default aggregates: %s", why[0] ? why : preAlps_hip_last_error());
    }
  }
  double* d = (double*)pa_rt_malloc((size_t)cnt * sizeof(double));
  if (!d || !h) {        /* nothing to hand to the hook: this process fails alone, as in pa_ranks_agree */
    if (!rc) snprintf(err, errlen, "no device buffer for the default aggregates: %s", pa_rt_error());
    free(loc); free(h); pa_rt_free(d);
    return 1;
  }
  if (rc) h[3 * me + 2] = 1.0;
  else {
    h[3 * me] = nloc; h[3 * me + 1] = npl;
    for (int q = 0; q < npl; ++q) h[3 * W + op->part0 + q] = loc[q];
  }
  const int up = pa_rt_h2d(d, h, (size_t)cnt * sizeof(double));
  const int comm_bad = pa_allreduce(d, cnt) || up || pa_rt_d2h(h, d, (size_t)cnt * sizeof(double));
  pa_rt_free(d);
  if (comm_bad) {       /* (not settled: left to the caller's next agreement) */
    if (!rc) { rc = 1; snprintf(err, errlen, "assembling the default aggregates over the processes failed: %s", pa_rt_error()); }
  } else {
    int failed = 0, parts = 0;
    for (int r = 0; r < W; ++r) { failed += h[3 * r + 2] != 0.0; parts += (int)h[3 * r + 1]; }
    if (failed || parts != npg) {       /* every process reads the same sums */
      *settled = 1;
      if (!rc) { rc = 1; snprintf(err, errlen, failed ? BJC_OTHER : "the processes hold %d parts of %d", parts, npg); }
    }
  }
  if (!rc) {
    int p = 0, g0 = 0;
    for (int r = 0; r < W; ++r) {
      const int na = (int)h[3 * r], np_r = (int)h[3 * r + 1];
      if (r == me && p != op->part0) {      /* (the parts are owned rank after rank; left to the caller's next agreement) */
        rc = 1; snprintf(err, errlen, "this process owns the parts from %d, the counts of the others put it at %d", op->part0, p);
      }
      for (int q = 0; q < np_r; ++q, ++p) co->part_aggregate[p] = g0 + (int)h[3 * W + p];
      g0 += na;
    }
    co->naggr = g0;
  }
  free(loc); free(h);
  return rc;
}

int preAlps_BlockJacobiSetCoarseSpace(int k, const double* V, int ldv, const int* part_aggregate, int naggr) {
  pa_bj_t* s = pa_bj_state();
  const double t0 = pa_wtime();
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return BJC_FAIL("operator not built");
  const int multi = bjc_multi();
  char err[320];
  err[0] = 0;
  int rc = bjc_args(s, op, k, V, ldv, part_aggregate, naggr, err, sizeof(err));
  if (!multi) { if (rc) return BJC_FAIL("%s", err); }
  else if (pa_ranks_agree(rc, NULL)) return BJC_FAIL("%s", rc ? err : BJC_OTHER);

  pa_bj_coarse_t co;
  memset(&co, 0, sizeof(co));
  const int N = op->N, npg = op->nparts;
  int settled = 0;
  co.k = k; co.n = N; co.nparts = npg; co.multi = multi;
  co.V = (double*)malloc((size_t)N * k * sizeof(double));
  co.part_aggregate = (int*)malloc((size_t)npg * sizeof(int));
  if (!co.V || !co.part_aggregate) {
    if (!multi) { pa_bj_coarse_release(&co); return BJC_FAIL("out of host memory for the %d vectors", k); }
    rc = 1; snprintf(err, sizeof(err), "out of host memory for the %d vectors", k);
  }
  if (!rc) for (int a = 0; a < k; ++a) memcpy(co.V + (size_t)a * N, V + (size_t)a * ldv, (size_t)N * sizeof(double));
  if (part_aggregate) {
    if (!rc) memcpy(co.part_aggregate, part_aggregate, (size_t)npg * sizeof(int));
    co.naggr = naggr;
  } else if (!multi) {
    int* rp = (int*)malloc(((size_t)npg + 1) * sizeof(int));
    if (!rp) { pa_bj_coarse_release(&co); return BJC_FAIL("out of host memory"); }
    for (int q = 0; q <= npg; ++q) rp[q] = op->rowPos[op->part0 + q] - op->row_off;
    pa_coarse_in_t in = {.m = op->m, .nparts = npg, .rowPtr = op->A.rowPtr, .lcol = op->A.colInd, .val = op->A.val,
                         .rowPos = rp, .k = k, .max_dofs = PA_COARSE_MAX_DOFS};
    rc = pa_coarse_default_aggregates(&in, preAlps_hip_partition_kway, co.part_aggregate, &co.naggr, err, sizeof(err));
    free(rp);
    if (rc) { pa_bj_coarse_release(&co); return BJC_FAIL("default aggregates: %s", err[0] ? err : preAlps_hip_last_error()); }
  } else {
    rc = bjc_default_ranks(s, op, &co, rc, &settled, err, sizeof(err));
    if (rc && settled) { pa_bj_coarse_release(&co); return BJC_FAIL("%s", err); }
  }
  pa_coarse_t hc;
  rc = bj_coarse_form(s, &co, op, &hc, rc, &settled, err, sizeof(err));
  if (rc && settled) { pa_bj_coarse_release(&co); return BJC_FAIL("%s", err); }
  size_t b_ei = 0;
  if (!rc) {
    co.naggr = hc.naggr; co.nc = hc.nc; co.nchunks = hc.nchunks; co.nrows = hc.nrows;
    const size_t m = (size_t)op->m, nch = (size_t)(hc.nchunks ? hc.nchunks : 1), nc = (size_t)hc.nc;
    const size_t b_zv = m * k * sizeof(double), b_ch = nch * sizeof(int), b_ap = ((size_t)hc.naggr + 1) * sizeof(int),
                 b_pa = nch * k * 16 * sizeof(double), b_cy = nc * 16 * sizeof(double),
                 b_ro = multi ? (size_t)(hc.nrows ? hc.nrows : 1) * sizeof(int) : 0;
    b_ei = (multi ? (size_t)(hc.nrows ? hc.nrows : 1) : nc) * nc * sizeof(double);
    co.d_zv = (double*)pa_rt_malloc(b_zv);
    co.d_ch_row0 = (int*)pa_rt_malloc(b_ch); co.d_ch_nrows = (int*)pa_rt_malloc(b_ch); co.d_ch_aggr = (int*)pa_rt_malloc(b_ch);
    co.d_agg_ptr = (int*)pa_rt_malloc(b_ap); co.d_agg_chunk = (int*)pa_rt_malloc(b_ch);
    co.d_Einv = (double*)pa_rt_malloc(b_ei); co.d_partial = (double*)pa_rt_malloc(b_pa);
    co.d_c = (double*)pa_rt_malloc(b_cy); co.d_y = (double*)pa_rt_malloc(b_cy);
    if (multi) co.d_rows = (int*)pa_rt_malloc(b_ro);
    if (!co.d_zv || !co.d_ch_row0 || !co.d_ch_nrows || !co.d_ch_aggr || !co.d_agg_ptr || !co.d_agg_chunk || !co.d_Einv ||
        !co.d_partial || !co.d_c || !co.d_y || (multi && !co.d_rows) ||
        pa_rt_h2d(co.d_ch_row0, hc.ch_row0, b_ch) || pa_rt_h2d(co.d_ch_nrows, hc.ch_nrows, b_ch) ||
        pa_rt_h2d(co.d_ch_aggr, hc.ch_aggr, b_ch) || pa_rt_h2d(co.d_agg_ptr, hc.agg_ptr, b_ap) ||
        pa_rt_h2d(co.d_agg_chunk, hc.agg_chunk, b_ch) || (multi && pa_rt_h2d(co.d_rows, hc.rows, b_ro)) ||
        bj_coarse_upload(&co, &hc) ||
        pa_rt_memset(co.d_partial, 0, b_pa) || pa_rt_memset(co.d_c, 0, b_cy) || pa_rt_memset(co.d_y, 0, b_cy) || pa_rt_sync()) {
      rc = 1;
      snprintf(err, sizeof(err), "uploading the coarse space (%zu bytes of Einv) failed: %s", b_ei, pa_rt_error());
    }
    co.bytes = (double)(b_zv + 4 * b_ch + b_ap + b_ei + b_pa + 2 * b_cy + b_ro);
    pa_coarse_free(&hc);
  }
  if (multi && pa_ranks_agree(rc, NULL) && !rc) { rc = 1; snprintf(err, sizeof(err), BJC_OTHER); }
  if (rc) { pa_bj_coarse_release(&co); return BJC_FAIL("%s", err); }
  co.plan = (pa_coarse_plan_t){.m = op->m, .k = k, .naggr = co.naggr, .nc = co.nc, .nchunks = co.nchunks, .zv = co.d_zv,
                               .ch_row0 = co.d_ch_row0, .ch_nrows = co.d_ch_nrows, .ch_aggr = co.d_ch_aggr,
                               .agg_ptr = co.d_agg_ptr, .agg_chunk = co.d_agg_chunk, .Einv = co.d_Einv,
                               .partial = co.d_partial, .c = co.d_c, .y = co.d_y, .nrows = co.nrows, .rows = co.d_rows};
  co.on = 1; co.builds = 1;
  co.setup_s = pa_wtime() - t0;
  pa_bj_coarse_release(&s->co);     /* setting a coarse space again replaces it (the copies above have drained the stream) */
  s->co = co;
  pa_bj_apply_epoch_bump();
  return 0;
}

/* The coarse space follows the new values and the new scaling vector: zv, E and Einv formed again from the kept V and
 * aggregates and written into the same device arrays (the chunk lists depend on the partition alone).  A singular E
 * drops the coarse space; the block factor is not touched here.  Several processes: collective like the attach, and
 * what one process meets drops the coarse space on all. */
int pa_bj_coarse_refresh(pa_bj_t* s, const pa_operator_info_t* op) {
  pa_bj_coarse_t* co = &s->co;
  const double t0 = pa_wtime();
  char err[320];
  err[0] = 0;
  pa_coarse_t hc;
  int settled = 0;
  int rc = bj_coarse_form(s, co, op, &hc, 0, &settled, err, sizeof(err));
  if (!rc && (hc.nc != co->nc || hc.nchunks != co->nchunks || hc.nrows != co->nrows)) {
    rc = 1; snprintf(err, sizeof(err), "the partition changed"); pa_coarse_free(&hc);
  }
  if (!rc) {
    if (bj_coarse_upload(co, &hc)) { rc = 1; snprintf(err, sizeof(err), "uploading it failed: %s", pa_rt_error()); }
    pa_coarse_free(&hc);
  }
  if (co->multi && !(rc && settled) && pa_ranks_agree(rc, NULL) && !rc) { rc = 1; snprintf(err, sizeof(err), BJC_OTHER); }
  if (rc) {
    if (pa_rt_sync()) { /* nothing more to report */ }
    pa_bj_coarse_release(co);
    pa_bj_apply_epoch_bump();
    return BJU_FAIL("the coarse space was dropped, the refreshed block factor stays: %s", err);
  }
  ++co->builds;
  co->setup_s = pa_wtime() - t0;
  return 0;
}
