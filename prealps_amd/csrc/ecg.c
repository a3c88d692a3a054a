/*
 * ecg.c -- Enlarged Conjugate Gradient, reverse-communication state machine,
 * with every panel resident in HBM and every O(m) operation a HIP kernel.
 *
 * Reference behaviour kept (src/solvers/ecg.c under /root/reference):
 *   _preAlps_ECGMalloc          :41-96     one pool, V | AV | Z | R | X | small
 *   _preAlps_ECGReset / Split   :98-171, :201-221
 *   preAlps_ECGInitialize       :173-199   (size >= enlFac check on nparts)
 *   preAlps_ECGStoppingCriterion:223-271   Frobenius norm of the residual block
 *   _preAlps_ECGIterateOmin     :289-400   incl. BF-Omin (dpstrf / dlapmt)
 *   _preAlps_ECGIterateOdir     :402-530   incl. D-Odir (dgesvd / dgeqrf / dormqr)
 *   _preAlps_ECGIterateOdirFused:532-658   one reduction per iteration
 *   preAlps_ECGFinalize/WrapUp/Free :660-692, preAlps_ECGPrint :694-728
 *
 * MI355X design instead of the reference's:
 *   - panels are row-interleaved [m][ts] so one CSR gather touches one 8*ts-byte
 *     chunk; descriptors say ROW_MAJOR with lda = ts and hold device pointers;
 *   - without block-size reduction the three mkl_domatcopy per iteration
 *     (ecg.c:521-523) are pointer rotations among the P / P_prev / Z buffers;
 *   - t x t blocks stay on the device (Gram partials -> fixed-order finish ->
 *     all-reduce hook -> one-wave Cholesky); the host only reads the residual
 *     norm once per iteration, inside preAlps_ECGStoppingCriterion.
 */
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ecg_priv.h"
#include "smalldense.h"

_Static_assert((int)PA_ECG_ORTHOMIN == (int)ORTHOMIN && (int)PA_ECG_ORTHODIR == (int)ORTHODIR &&
               (int)PA_ECG_ORTHODIR_FUSED == (int)ORTHODIR_FUSED && (int)PA_ECG_ADAPT_BS == (int)ADAPT_BS &&
               (int)PA_ECG_NO_BS_RED == (int)NO_BS_RED, "ecg_plan.h restates the enums of preAlps_abi.h");

/* 1: the driver loops of this library (preAlps_ECGSolve / preAlps_ECGAdvance) replay the launches of
 * an iteration from HIP graphs captured on the first passes (see seg_begin in ecg_loops.c); -1 = decide from
 * PREALPS_ECG_GRAPH (default 0) at the next reset. */
static int g_graphs = -1;
/* > 0 inside preAlps_ECGSolve / preAlps_ECGAdvance.  Only there does the library ask its SpMM and its block
 * solve for the Gram blocks of the next half-iteration: between preAlps_BlockOperator / BlockJacobiApply and
 * preAlps_ECGIterate nothing else touches AP or Z in those loops, whereas a caller that drives the RCI
 * protocol itself may (a shifted operator, a second preconditioner stage), and the blocks would be stale.
 * PREALPS_RCI_FUSE=1: also for RCI callers who only call the two library routines. */
static int g_own_loop = 0;
static int rci_fuse(void) { static int v = -1; if (v < 0) { const char* e = getenv("PREALPS_RCI_FUSE"); v = e ? atoi(e) : 0; } return v; }
void preAlps_hip_graphs(int on) { g_graphs = on; }
int pa_ecg_in_own_loop(void) { return g_own_loop; }
void pa_ecg_enter_own_loop(void) { ++g_own_loop; }
void pa_ecg_leave_own_loop(void) {
  if (--g_own_loop == 0) { pa_k_spmm_gram_disarm(NULL); pa_k_bj_gram_disarm(NULL); }
}

static void publish_pointers(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  ecg->V->val = pv->buf_v[0];
  ecg->AV->val = pv->buf_av[0];
  ecg->P->val = pv->buf_v[0];
  ecg->AP->val = pv->buf_av[0];
  ecg->Z->val = pv->buf_z;
  ecg->R->val = pv->d_R;
  ecg->X->val = pv->d_X;
  ecg->alpha->val = pv->d_alpha;
  ecg->beta->val = pv->d_beta;
  ecg->P_p = pv->buf_v[0];
  ecg->AP_p = pv->buf_av[0];
  ecg->R_p = pv->d_R;
  ecg->Z_p = pv->buf_z;
}

/* the direction panels in the initial order of the pool (pv->lay) */
static void place_panels(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  const pa_ecg_pool_t* lay = &pv->lay;
  double* w = ecg->work;
  pv->buf_v[0] = w + lay->v[0];
  pv->buf_v[1] = lay->v[1] != PA_ECG_ABSENT ? w + lay->v[1] : NULL;
  pv->buf_av[0] = w + lay->av[0];
  pv->buf_av[1] = lay->av[1] != PA_ECG_ABSENT ? w + lay->av[1] : NULL;
  pv->buf_z = w + lay->z;
}

static int pa_env_flag(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static int solve_first_switch(void) { return pa_env_flag("PREALPS_ECG_SOLVE_FIRST", 1); }

int preAlps_hip_ecg_solve_first(int nprocs, int ortho_alg, int bs_red, int enlFac, int fuse, int lazy_norm,
                                int lazy_stop, int bj_gram, int spmm_gram, int graphs) {
  return pa_ecg_solve_first_rule(solve_first_switch(), nprocs, ortho_alg, bs_red, enlFac, fuse, lazy_norm, lazy_stop,
                                 bj_gram, spmm_gram, graphs);
}

/* ------------------------------------------------------------- malloc ---- */
int _preAlps_ECGMalloc(preAlps_ECG_t* ecg) {
  PA_REQUIRE_GPU();
  int m = ecg->locPbSize, T = ecg->enlFac;
  if (T < 1 || T > 16) return PA_FAIL("enlarging factor %d outside the supported range 1..16", T);
  int ts = pa_panel_stride(T);
  ecg->X = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->R = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->V = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->AV = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->Z = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->alpha = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->beta = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->P = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  ecg->AP = (CPLM_Mat_Dense_t*)calloc(1, sizeof(CPLM_Mat_Dense_t));
  int skip = (T + 3) & ~3;
  ecg->iwork = (int*)calloc(1, skip * sizeof(int) + sizeof(ecg_priv_t));
  ecg_priv_t* pv = (ecg_priv_t*)(ecg->iwork + skip);
  pv->magic = PA_ECG_MAGIC; pv->ts = ts; pv->T = T; pv->m = m;
  /* T = 4: the library's SpMM can form [AP | R]^T P while it computes AP (one block per workgroup) */
  pv->spmm_cap = (T == 4 && ts == 4) ? pa_operator_gram_blocks(ts) : 0;
  /* ... and the library's block solve beta = [AP | AP_prev]^T Z while Z is still in its registers (Orthodir) */
  pv->bj_cap = (T == 4 && ts == 4 && ecg->ortho_alg == ORTHODIR && pa_env_flag("PREALPS_BJ_GRAM", 1)) ? pa_bj_gram_blocks() : 0;
  const pa_ecg_pool_in_t in = {.m = m, .T = T, .ts = ts, .ortho_alg = ecg->ortho_alg, .spmm_cap = pv->spmm_cap,
                               .bj_cap = pv->bj_cap, .G = pa_gram_max_blocks(), .S = pa_finish32_scratch_blocks()};
  const pa_ecg_pool_t* lay = &pv->lay;
  pa_ecg_pool_layout(&in, &pv->lay);
  ecg->work = (double*)pa_rt_malloc(lay->pool_doubles * sizeof(double));
  if (!ecg->work) return PA_FAIL("device pool of %zu doubles: %s", lay->pool_doubles, pa_rt_error());
  double* w = ecg->work;
  place_panels(ecg, pv);
  pv->d_R = w + lay->r; pv->d_X = w + lay->x;
  pv->d_F = w + lay->F; pv->d_alpha = w + lay->alpha; pv->d_beta = w + lay->beta; pv->d_mu = w + lay->mu;
  pv->d_rtr = w + lay->rtr;
  pv->d_q = w + lay->q;
  pv->d_res2 = w + lay->res2;
  pv->d_uu = w + lay->uu;
  pv->d_partials = w + lay->partials;
  pv->d_rtr_part = w + lay->rtr_part;
  pv->d_spmm_parts = pv->spmm_cap ? w + lay->spmm_parts : NULL;
  pv->d_bj_parts = pv->bj_cap ? w + lay->bj_parts : NULL;
  pv->d_grp = w + lay->grp;
  pv->d_sys_part = w + lay->sys_part;
  pv->d_info = (int*)pa_rt_malloc((8 + T) * sizeof(int));
  if (!pv->d_info) return PA_FAIL("device allocation failed: %s", pa_rt_error());
  pv->d_piv = pv->d_info + 8;
  pv->d_akeep = (double*)pa_rt_malloc(2 * (size_t)T * T * sizeof(double));    /* (not in the pool: see ecg_priv.h) */
  if (!pv->d_akeep) return PA_FAIL("device allocation failed: %s", pa_rt_error());
  pv->h_pin = (double*)pa_rt_host_alloc_coherent((16 + 4 * (size_t)T * T) * sizeof(double));
  pv->h_pin_i = (int*)pa_rt_host_alloc((8 + T) * sizeof(int));
  pv->h_grp = (double*)pa_rt_host_alloc_coherent(48 * sizeof(double));
  if (!pv->h_pin || !pv->h_pin_i || !pv->h_grp) return PA_FAIL("pinned allocation failed: %s", pa_rt_error());
  pv->ev_res = pa_rt_event_create();
  pv->ev_alpha = pa_rt_event_create();
  if (!pv->ev_res || !pv->ev_alpha) return PA_FAIL("hipEventCreate failed");
  publish_pointers(ecg, pv);
  return 0;
}

/* The first half of the next iteration starts with [AP | R]^T P (fused_first_half): when the
 * product P -> AP is the library's SpMM on 4-column panels, ask it to leave that block behind.
 * Called whenever the P / AP pointers have been published; anything else ends the request. */
void pa_ecg_request_gram_from_spmm(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  if ((g_own_loop > 0 || rci_fuse()) && pv->spmm_cap > 0 && pv->fuse && ecg->bs_red == NO_BS_RED &&
      ecg->ortho_alg != ORTHODIR_FUSED && ecg->enlFac == 4 && ecg->P->info.n == 4)
    pa_k_spmm_gram_arm(ecg->P->val, ecg->AP->val, pv->d_R, pv->d_spmm_parts, pv->spmm_cap);
  else if (pv->d_spmm_parts)
    pa_k_spmm_gram_disarm(pv->d_spmm_parts);
}

/* ------------------------------------------------------------- reset ---- */
/* Everything of a reset but R0 and the norm of the right-hand side: timers, pointer order, the switches, the
 * descriptors, the zeroed pool.  nrhs: the systems the solver will hold (1 from _preAlps_ECGReset); guess: it starts
 * from an initial guess; metric: its stopping test is the caller's (preAlps_ECGSolveSystem). */
int pa_ecg_reset_state(preAlps_ECG_t* ecg, ecg_priv_t* pv, int nrhs, int guess, int metric) {
  pv->nrhs = nrhs; pv->sgrp = ecg->enlFac / nrhs; pv->guess = guess; pv->metric = metric; pv->d_dl = NULL;
  pv->grp_dst = NULL;
  pv->energy = NULL; pv->energy_stop = 0;
  ecg->tot_t = ecg->comm_t = ecg->trsm_t = ecg->gemm_t = ecg->potrf_t = ecg->pstrf_t = 0.0;
  ecg->lapmt_t = ecg->gesvd_t = ecg->geqrf_t = ecg->ormqr_t = ecg->copy_t = 0.0;
  int M = ecg->globPbSize, m = ecg->locPbSize, t = ecg->enlFac, ts = pv->ts;
  /* pointer order back to the initial one */
  place_panels(ecg, pv);
  publish_pointers(ecg, pv);
  /* the switches, as they stand at this reset (the rules and their reasons: pa_ecg_switches) */
  const int poll = pa_env_flag("PREALPS_ECG_POLL", INT_MIN);   /* (INT_MIN: no value of the switch, so it tells unset) */
  const pa_ecg_switch_in_t in = {
    .ortho_alg = ecg->ortho_alg, .bs_red = ecg->bs_red, .enlFac = ecg->enlFac, .nrhs = nrhs, .guess = guess, .metric = metric,
    .world = pa_world_size(), .loopback = pa_comm_is_loopback(), .timing = pa_timing_enabled(),
    .fuse = pa_env_flag("PREALPS_ECG_FUSE", 1), .lazy_norm = pa_env_flag("PREALPS_ECG_LAZY_NORM", 1),
    .lazy_stop = pa_env_flag("PREALPS_ECG_LAZY_STOP", 1),
    .graphs = g_graphs >= 0 ? g_graphs : pa_env_flag("PREALPS_ECG_GRAPH", 0),
    .poll = poll == INT_MIN ? -1 : poll != 0};
  pa_ecg_switch_t sw;
  pa_ecg_switches(&in, &sw);
  pv->rotate = sw.rotate; pv->fuse = sw.fuse; pv->lazy_norm = sw.lazy_norm; pv->lazy_stop = sw.lazy_stop;
  pv->use_graphs = sw.use_graphs; pv->poll = sw.poll; pv->ride = sw.ride; pv->ride_sys = sw.ride_sys;
  pv->solve_first = solve_first_switch();
  pv->x_defer = pa_env_flag("PREALPS_ECG_X_DEFER", 1) != 0;
  pv->x_pending = 0;
  pv->uu_cur = 0;
  pv->z_ready = 0;
  pv->sf_ready = 0;
  pv->lazy_ptr = NULL;
  pv->phase = 0;
  pv->sent_seq = pv->wait_seq = 0.0;
  if (pv->h_pin) pv->h_pin[2] = 0.0;
  pa_set_desc(ecg->X, M, t, m, t, ts);
  pa_set_desc(ecg->R, M, t, m, t, ts);
  pa_set_desc(ecg->Z, M, t, m, t, ts);
  if (ecg->ortho_alg == ORTHOMIN) {
    pa_set_desc(ecg->V, M, t, m, t, ts);
    pa_set_desc(ecg->AV, M, t, m, t, ts);
    CPLM_MatDenseSetInfo(ecg->alpha, t, t, t, t, COL_MAJOR);
    CPLM_MatDenseSetInfo(ecg->beta, t, t, t, t, COL_MAJOR);
  } else {
    pa_set_desc(ecg->V, M, 2 * t, m, 2 * t, ts);
    pa_set_desc(ecg->AV, M, 2 * t, m, 2 * t, ts);
    CPLM_MatDenseSetInfo(ecg->alpha, t, t, t, t, COL_MAJOR);
    CPLM_MatDenseSetInfo(ecg->beta, 2 * t, t, 2 * t, t, COL_MAJOR);
  }
  pa_set_desc(ecg->P, M, t, m, t, ts);
  pa_set_desc(ecg->AP, M, t, m, t, ts);
  PA_CHECK(pa_rt_memset(ecg->work, 0, pv->lay.pool_doubles * sizeof(double)));
  if (pv->lazy_norm) {        /* (the first update meets an empty P_prev: any factor will do, the identity is one) */
    double eye[2 * 16 * 16];
    memset(eye, 0, sizeof(eye));
    for (int k = 0; k < 2; ++k) for (int i = 0; i < t; ++i) eye[(size_t)k * t * t + i + (size_t)t * i] = 1.0;
    PA_CHECK(pa_rt_h2d(pv->d_uu, eye, 2 * (size_t)t * t * sizeof(double)));
  }
  return 0;
}
void pa_ecg_reset_done(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* rci_request) {
  ecg->res = 1.0; ecg->iter = 0; ecg->bs = ecg->enlFac; ecg->kbs = ecg->V->info.n;
  pv->rtr_valid = RTR_NONE;
  *rci_request = 0;
  pa_ecg_request_gram_from_spmm(ecg, pv);
}

int _preAlps_ECGReset(preAlps_ECG_t* ecg, double* rhs, int* rci_request) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver memory not allocated (_preAlps_ECGMalloc)");
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built before the solver");
  if (ecg->locPbSize != op->m) return PA_FAIL("locPbSize %d differs from the operator's %d rows", ecg->locPbSize, op->m);
  if (pv->nrhs > 1) return PA_FAIL("the solver holds %d systems: restart it with preAlps_ECGInitializeMulti", pv->nrhs);
  if (pa_ecg_reset_state(ecg, pv, 1, 0, 0)) return 1;
  int m = ecg->locPbSize, t = ecg->enlFac, ts = pv->ts;
  /* normb and R0: column (rank % t) of every reference rank = part */
  double nb2 = 0.0;
  double* r0 = (double*)calloc((size_t)(m > 0 ? m : 1) * ts, sizeof(double));
  if (!r0) return PA_FAIL("out of host memory");
  for (int p = op->part0; p < op->part1; ++p) {
    int base = op->rowPos[p] - op->row_off, l = op->rowPos[p + 1] - op->rowPos[p];
    int col = p % t;
    double s = 0.0;
    for (int i = 0; i < l; ++i) { double v = rhs[base + i]; s += v * v; r0[(size_t)(base + i) * ts + col] = v; }
    nb2 += s;
  }
  int rc = pa_rt_h2d(pv->d_R, r0, (size_t)m * ts * sizeof(double));
  free(r0);
  if (rc) return PA_FAIL("%s", pa_rt_error());
  if (pa_world_size() > 1) {
    double t0;
    TIC(PA_T_COMM);
    PA_CHECK(pa_rt_h2d(pv->d_res2, &nb2, sizeof(double)));
    if (pa_allreduce(pv->d_res2, 1)) return 1;
    PA_CHECK(pa_rt_d2h(&nb2, pv->d_res2, sizeof(double)));
    TAC(PA_T_COMM, comm_t);
  }
  ecg->normb = sqrt(nb2);
  pa_ecg_reset_done(ecg, pv, rci_request);
  return 0;
}

int preAlps_ECGInitialize(preAlps_ECG_t* ecg, double* rhs, int* rci_request) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built before the solver");
  /* ecg.c:178-183 with the reference's "processors" = subdomains */
  if (op->nparts < ecg->enlFac)
    return PA_FAIL("Enlarging factor must be lower than the number of processors"
                   " in the MPI communicator! size: %d ; enlarging factor: %d", op->nparts, ecg->enlFac);
  int rc = _preAlps_ECGMalloc(ecg);
  if (rc) return rc;
  return _preAlps_ECGReset(ecg, rhs, rci_request);
}

int _preAlps_ECGSplit(double* x, CPLM_Mat_Dense_t* XSplit, int colIndex) {
  if (!XSplit || !XSplit->val || !x) return PA_FAIL(" wrong test 'XSplit->val != NULL && x != NULL'");
  int m = XSplit->info.m, ts = pa_desc_stride(XSplit);
  double* tmp = (double*)malloc((size_t)(m > 0 ? m : 1) * ts * sizeof(double));
  if (!tmp) return PA_FAIL("out of host memory");
  int rc = pa_rt_d2h(tmp, XSplit->val, (size_t)m * ts * sizeof(double));
  for (int i = 0; i < m; ++i) tmp[(size_t)i * ts + colIndex] = x[i];
  rc = rc || pa_rt_h2d(XSplit->val, tmp, (size_t)m * ts * sizeof(double));
  free(tmp);
  if (rc) return PA_FAIL("%s", pa_rt_error());
  return 0;
}

/* ---------------------------------------------------------- stopping ---- */
/* The stopping test in two halves: `begin` queues the reduction of the residual
 * norm and its copy to pinned host memory and marks that point with an event;
 * `end` waits for the event only -- not for the stream -- so work queued after
 * `begin` (the preconditioner apply of the same iteration) keeps the GPU busy
 * while the host reads the norm. */
/* Several systems: the per-system sums, right behind the launch that left the column sums in d_rtr_part (rtr_nblk
 * blocks) and so ahead of whatever carries the scalar norm to the host. */
/* The caller's metric: the R panel itself is read instead -- every call site comes behind the launch that wrote this
 * iteration's R, on the same stream (the update kernels of fused_update, update_iterate and solve_first_step; in
 * stopping_queue nothing has touched R since); R never takes part in the rotation of the direction panels, and its
 * pointer is taken from the descriptor at the moment of the launch. */
/* Several processes (pv->ride, and with the caller's metric pv->ride_sys): the sums are local, and go behind the pair
 * [norm^2, status] at `dst` that the next collective carries (d_res2, or the slot behind beta when the norm is summed
 * with beta); dst is unused otherwise. */
int pa_ecg_queue_group_norms(preAlps_ECG_t* ecg, ecg_priv_t* pv, double* dst) {
  if (pv->ride) {
    PA_CHECK(pa_k_group_norms_ride(pv->d_rtr_part, pv->rtr_nblk, pv->ts, pv->nrhs, pv->sgrp, pv->d_info, dst));
    pv->grp_dst = dst;
  } else if (pv->metric) {
    int nb = 0;
    const int k = pv->nrhs > 1 ? pv->nrhs : 1;
    PA_CHECK(pa_k_sys_norms(pv->m, pv->ts, k, pv->sgrp, ecg->R->val, pv->d_dl, pv->d_sys_part, &nb));
    if (pv->ride_sys) {
      /* several processes: this process's share, folded behind the pair at dst with the scaled norm of all of R */
      PA_CHECK(pa_k_sys_norms_ride(pv->d_rtr_part, pv->rtr_nblk, pv->d_sys_part, nb, pv->ts, k, pv->sgrp, pv->d_info, dst));
      pv->grp_dst = dst;
    } else
      PA_CHECK(pa_k_group_norms(pv->d_sys_part, nb, pv->ts, k, 1, pv->d_grp, pv->h_grp));
  } else if (pv->nrhs > 1)
    PA_CHECK(pa_k_group_norms(pv->d_rtr_part, pv->rtr_nblk, pv->ts, pv->nrhs, pv->sgrp, pv->d_grp, pv->h_grp));
  return 0;
}
int pa_ecg_stopping_queue(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  int T = ecg->enlFac;
  int single = pa_world_size() == 1;
  if (pa_ecg_rides(pv)) {
    /* several systems, or the caller's metric, on several processes: pa_k_group_norms_ride / pa_k_sys_norms_ride has left [norm^2, status | g_0^2 .. g_k-1^2] of
     * this process at grp_dst behind the last update (from R itself when nothing is left of one); ONE all-reduce
     * of 2 + k words where one system reduces its norm, and the k global sums follow the pair to the host */
    if (pv->rtr_valid == RTR_NONE) {
      PA_CHECK(pa_k_colnorm2(pv->m, pv->ts, pv->d_R, pv->d_rtr_part, &pv->rtr_nblk));
      if (pa_ecg_queue_group_norms(ecg, pv, pv->d_res2)) return 1;
    }
    double* src = pv->grp_dst;
    double t0;
    TIC(PA_T_COMM);
    if (pa_allreduce(src, 2 + pv->nrhs)) return 1;
    TAC(PA_T_COMM, comm_t);
    PA_CHECK(pa_rt_d2h_async(pv->h_pin, src, 2 * sizeof(double)));
    PA_CHECK(pa_rt_d2h_async(pv->h_grp, src + 2, (size_t)pv->nrhs * sizeof(double)));
    pv->wait_seq = pv->sent_seq = 0.0;
    pv->rtr_valid = RTR_NONE;
    return 0;
  }
  if (pv->rtr_valid < RTR_SUMMED) {
    if (pv->rtr_valid == RTR_NONE) {
      PA_CHECK(pa_k_colnorm2(pv->m, pv->ts, pv->d_R, pv->d_rtr_part, &pv->rtr_nblk));
      if (pa_ecg_queue_group_norms(ecg, pv, NULL)) return 1;
    }
    if (single && pv->rtr_valid == RTR_COLUMN_SUMS) {
      /* column sums left by the update kernel (lazy stopping test), one process: the sum goes straight to
       * the pinned words, as it does from the update kernel's own launch without the lazy test */
      pv->sent_seq = 0.0;
      if (pv->poll) { pv->sent_seq = (pv->seq += 1.0); pa_k_note_seq(pv->sent_seq); }
      PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->d_res2, pv->d_info, pv->h_pin));
      pv->rtr_valid = RTR_SUMMED;
    } else {
      PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->d_res2, pv->d_info, NULL));
      pv->rtr_valid = RTR_ON_DEVICE;
    }
  }
  /* RTR_SUMMED: the update kernel summed the norm itself and, in a single-process run,
   * already wrote it to the pinned words the host reads */
  pv->wait_seq = 0.0;
  if (!single || pv->rtr_valid == RTR_ON_DEVICE) {
    double* src = (pv->rtr_valid == RTR_SUMMED && pv->lazy_ptr) ? pv->lazy_ptr : pv->d_res2;
    double t0;
    TIC(PA_T_COMM);
    if (pa_allreduce(src, 1)) return 1;
    TAC(PA_T_COMM, comm_t);
    PA_CHECK(pa_rt_d2h_async(pv->h_pin, src, 2 * sizeof(double)));
  } else {
    pv->wait_seq = pv->sent_seq;     /* the update kernel's launch writes the words and this number behind them */
  }
  pv->sent_seq = 0.0;
  pv->rtr_valid = RTR_NONE;
  return 0;
}
int pa_ecg_stopping_begin(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  if (pa_ecg_stopping_queue(ecg, pv)) return 1;
  if (pv->wait_seq == 0.0) PA_CHECK(pa_rt_event_record(pv->ev_res));
  return 0;
}
/* Wait for the sequence number behind the two pinned words (see _preAlps_ECGReset). */
static int wait_for_note(ecg_priv_t* pv) {
  volatile double* h = pv->h_pin;
  double t0 = pa_wtime();
  unsigned long spins = 0;
  int idle_seen = 0;
  while (h[2] != pv->wait_seq) {
    __builtin_ia32_pause();
    if ((++spins & 0x3fff) == 0) {
      int st = pa_rt_stream_state();
      if (st < 0) return PA_FAIL("%s", pa_rt_error());
      if (st == 1 && idle_seen++ > 2) return PA_FAIL("the residual norm never reached the host (stream idle)");
      if (pa_wtime() - t0 > 60.0) return PA_FAIL("timed out waiting for the residual norm");
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  pv->wait_seq = 0.0;
  return 0;
}

int pa_ecg_stopping_end(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* stop) {
  if (pv->wait_seq != 0.0) { if (wait_for_note(pv)) return 1; }
  else PA_CHECK(pa_rt_event_wait(pv->ev_res));
  double res2 = pv->h_pin[0];
  int info = (int)pv->h_pin[1];
  if (info != 0 && ecg->ortho_alg == ORTHOMIN) return PA_FAIL("ACHQR: dpotrf:\n ERROR: P^tAP is not spd!");
  ecg->res = sqrt(res2);
  /* the energy-norm drops of this iteration lie in the pinned words behind the same event; e_on: the verdict of the
   * tracker's rule where that is the test (1: on, 0: stop -- a drop that is not finite stops), -1 where it is not */
  int e_on = -1;
  if (pv->energy) {
    double drops[PA_ENERGY_MAX_SYSTEMS];
    const volatile double* h = pv->h_drop;
    for (int j = 0; j < (pv->nrhs > 1 ? pv->nrhs : 1); ++j) drops[j] = h[j];
    const int prc = pa_energy_push(pv->energy, drops);
    if (prc != PA_ENERGY_OK && prc != PA_ENERGY_NAN)
      return PA_FAIL("the energy-norm tracker took no drops at iteration %d (%s)", ecg->iter,
                     prc == PA_ENERGY_FULL ? "it is full" : "bad arguments");
    if (pv->energy_stop) e_on = pa_energy_goes_on(pv->energy, ecg->tol);
  }
  if (pv->nrhs > 1 || pv->metric) {
    /* every system against its own right-hand side: on while one of them is above its threshold; a NaN stops
     * (the caller's metric: for one system too, both sides in the caller's units) */
    int above = 0, nan = !(ecg->res == ecg->res);
    const int nsys = pv->nrhs > 1 ? pv->nrhs : 1;
    for (int j = 0; j < nsys; ++j) {
      const double g = sqrt(pv->h_grp[j]);
      pv->sys_res[j] = g;
      if (g > pv->sys_normb[j] * ecg->tol) above = 1;
      if (!(g == g)) nan = 1;
    }
    if (e_on >= 0) above = e_on;
    *stop = (above && !nan && ecg->iter < ecg->maxIter && ecg->bs > 0) ? 0 : 1;
    return 0;
  }
  /* !(a > b) also stops on NaN, like the reference's comparison */
  if ((e_on >= 0 ? e_on && ecg->res == ecg->res : ecg->res > ecg->normb * ecg->tol) && ecg->iter < ecg->maxIter && ecg->bs > 0) *stop = 0;
  else *stop = 1;
  return 0;
}

int preAlps_ECGStoppingCriterion(preAlps_ECG_t* ecg, int* stop) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  if (!stop) return PA_FAIL(" wrong test 'stop != NULL'");
  double tg = pa_wtime();
  if (pa_ecg_stopping_begin(ecg, pv)) return 1;
  if (pa_ecg_stopping_end(ecg, pv, stop)) return 1;
  ecg->tot_t += pa_wtime() - tg;
  return 0;
}

/* ------------------------------------------------------ shared pieces ---- */
/* W = AP^T P -> all-reduce -> U^T U ; P <- P U^-1 ; AP <- AP U^-1 ;
 * alpha = P^T R -> all-reduce   (ecg.c:311-333, :425-443) */
static int a_orthonormalise_and_alpha(preAlps_ECG_t* ecg, ecg_priv_t* pv, int t) {
  int m = pv->m, ts = pv->ts;
  double t0;
  TIC(PA_T_GRAM);
  PA_CHECK(pa_k_gram_finish(m, ts, ecg->AP->val, NULL, ecg->P->val, pv->d_partials, t, 0, t, pv->d_mu, t,
                            0, 0, NULL, NULL, NULL));
  TAC(PA_T_GRAM, gemm_t);
  TIC(PA_T_COMM);
  if (pa_allreduce(pv->d_mu, t * t)) return 1;
  TAC(PA_T_COMM, comm_t);
  TIC(PA_T_SMALL);
  PA_CHECK(pa_k_potrf(pv->d_mu, t, pv->d_info));
  TAC(PA_T_SMALL, potrf_t);
  TIC(PA_T_TRSM);
  PA_CHECK(pa_k_trsm(m, ts, t, pv->d_mu, ecg->P->val, ecg->AP->val));
  TAC(PA_T_TRSM, trsm_t);
  TIC(PA_T_GRAM);
  PA_CHECK(pa_k_gram_finish(m, ts, ecg->P->val, NULL, ecg->R->val, pv->d_partials, ecg->alpha->info.m, 0,
                            ecg->alpha->info.n, pv->d_alpha, ecg->alpha->info.lda, 0, 0, NULL, NULL, NULL));
  TAC(PA_T_GRAM, gemm_t);
  TIC(PA_T_COMM);
  if (pa_allreduce(pv->d_alpha, ecg->alpha->info.lda * ecg->alpha->info.n)) return 1;
  TAC(PA_T_COMM, comm_t);
  return 0;
}

/* The rci == 0 half without block-size reduction, in two passes over the panels
 * instead of four: [W ; G^T] = [AP | R]^T P (one Gram kernel, one all-reduce),
 * then U = chol(W), alpha = U^-T G on one wave, then P U^-1, AP U^-1, X += P alpha,
 * R -= AP alpha and the residual column norms in a single kernel.  Algebraically
 * ecg.c:425-443 + :500-501; alpha is formed from the Gram of the un-normalised P. */
static int fused_update(preAlps_ECG_t* ecg, ecg_priv_t* pv, int t, const double* gram);
static int fused_gram(preAlps_ECG_t* ecg, ecg_priv_t* pv, int t, int factor_now);
static int fused_first_half(preAlps_ECG_t* ecg, ecg_priv_t* pv, int t) {
  if (fused_gram(ecg, pv, t, 0)) return 1;
  return fused_update(ecg, pv, t, pa_world_size() == 1 ? NULL : pv->d_q);
}
/* first pass: [W ; G^T] summed over the processes in d_q; one process (or factor_now): U = chol(W) in d_mu and
 * alpha = U^-T G in d_alpha as well, so that the host can look at alpha before the panels are touched (D-Odir) */
static int fused_gram(preAlps_ECG_t* ecg, ecg_priv_t* pv, int t, int factor_now) {
  int m = pv->m, ts = pv->ts, T = ecg->enlFac;
  int single = pa_world_size() == 1;
  double* buf = pv->d_q; /* (t+T) x t */
  double t0;
  /* blocks the SpMM left behind while it formed AP (request_gram_from_spmm): only their sum is left to do */
  int from_spmm = pv->spmm_cap > 0 ? pa_k_spmm_gram_take(ecg->P->val, ecg->AP->val) : 0;
  TIC(PA_T_GRAM);
  if (single) {
    /* nothing to reduce across processes: the launch that sums the partial blocks factors them
     * right away */
    if (from_spmm) PA_CHECK(pa_k_finish32(pv->d_spmm_parts, from_spmm, pv->d_spmm_parts + (size_t)pv->spmm_cap * 32, t, T, buf,
                                         pv->d_mu, pv->d_alpha, pv->d_info));
    else PA_CHECK(pa_k_gram_finish(m, ts, ecg->AP->val, pv->d_R, ecg->P->val, pv->d_partials, t, T, t, buf, t + T,
                                   t, T, pv->d_mu, pv->d_alpha, pv->d_info));
    TAC(PA_T_GRAM, gemm_t);
  } else {
    if (from_spmm) PA_CHECK(pa_k_finish32(pv->d_spmm_parts, from_spmm, pv->d_spmm_parts + (size_t)pv->spmm_cap * 32, 0, 0, buf,
                                         NULL, NULL, NULL));
    else PA_CHECK(pa_k_gram_finish(m, ts, ecg->AP->val, pv->d_R, ecg->P->val, pv->d_partials, t, T, t, buf, t + T,
                                   0, 0, NULL, NULL, NULL));
    TAC(PA_T_GRAM, gemm_t);
    TIC(PA_T_COMM);
    if (pa_allreduce(buf, (t + T) * t)) return 1;
    TAC(PA_T_COMM, comm_t);
    /* (the factorisation of the reduced block and alpha: in the update kernel's prologue) */
    if (factor_now) {
      TIC(PA_T_SMALL);
      PA_CHECK(pa_k_potrf_alpha(buf, t, T, pv->d_mu, pv->d_alpha, pv->d_info));
      TAC(PA_T_SMALL, potrf_t);
    }
  }
  return 0;
}
/* second pass: P U^-1, AP U^-1, X += P alpha, R -= AP alpha and the residual column norms; gram != NULL: the
 * kernel's prologue factors the summed block first */
static int fused_update(preAlps_ECG_t* ecg, ecg_priv_t* pv, int t, const double* gram) {
  int nb = 0, m = pv->m, ts = pv->ts, T = ecg->enlFac;
  int single = pa_world_size() == 1;
  double t0;
  TIC(PA_T_UPDATE);
  /* the slot right behind beta: free once the kernel has read U from it (Odir: d_mu) */
  pv->lazy_ptr = pv->lazy_stop ? pv->d_beta + (size_t)ecg->beta->info.lda * ecg->beta->info.n : NULL;
  /* with the lazy stopping test the column sums of R^2 are added up by the launch that sums beta
   * (orthogonalise_z), next to which the norm travels: no launch of its own here */
  int defer = pv->lazy_ptr != NULL;
  pv->sent_seq = 0.0;
  if (single && pv->poll && !defer) { pv->sent_seq = (pv->seq += 1.0); pa_k_note_seq(pv->sent_seq); }
  PA_CHECK(pa_k_trsm_update(m, ts, t, ecg->X->info.n, pv->d_mu, pv->d_alpha, ecg->P->val, ecg->AP->val,
                            pv->d_X, pv->d_R, pv->d_rtr_part, &nb, defer ? 0 : T,
                            pv->lazy_ptr ? pv->lazy_ptr : pv->d_res2, pv->d_info, single ? pv->h_pin : NULL,
                            gram, pv->lazy_norm ? pv->d_uu + (size_t)pv->uu_cur * T * T : NULL));
  pv->rtr_nblk = nb;
  if (pa_ecg_queue_group_norms(ecg, pv, defer ? pv->lazy_ptr : pv->d_res2)) return 1;
  if (pa_ecg_queue_energy(ecg, pv)) return 1;
  TAC(PA_T_UPDATE, trsm_t);
  pv->rtr_valid = defer ? RTR_COLUMN_SUMS : RTR_SUMMED;
  return 0;
}

/* X += P alpha ; R -= AP alpha (ecg.c:337-338, :500-501) + residual norms */
static int update_iterate(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  double t0;
  TIC(PA_T_UPDATE);
  pv->sent_seq = 0.0;
  if (pa_world_size() == 1 && pv->poll) { pv->sent_seq = (pv->seq += 1.0); pa_k_note_seq(pv->sent_seq); }
  PA_CHECK(pa_k_update_xr(pv->m, pv->ts, ecg->P->info.n, ecg->X->info.n, pv->d_alpha, ecg->P->val,
                          ecg->AP->val, pv->d_X, pv->d_R, pv->d_rtr_part, &pv->rtr_nblk, ecg->enlFac,
                          pv->d_res2, pv->d_info, pa_world_size() == 1 ? pv->h_pin : NULL));
  if (pa_ecg_queue_group_norms(ecg, pv, pv->d_res2)) return 1;
  if (pa_ecg_queue_energy(ecg, pv)) return 1;
  TAC(PA_T_UPDATE, gemm_t);
  pv->rtr_valid = RTR_SUMMED;
  pv->lazy_ptr = NULL;
  return 0;
}

/* X every second row pass (ecg_priv.h: x_pending).  The debt is described by where the panels and the factors lie
 * AFTER the step that left it: pa_ecg_shift_directions has made its P the previous panel, and uu_cur has moved on. */
static long long g_x_skips, g_x_flushes;
long long pa_ecg_x_count(int which) { return which ? g_x_flushes : g_x_skips; }
void pa_ecg_x_owed(ecg_priv_t* pv) { pv->x_pending = 1; ++g_x_skips; }
int pa_ecg_flush_x(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  if (!pv->x_pending) return 0;
  const int T = ecg->enlFac;
  const size_t prev = (size_t)(1 - pv->uu_cur) * T * T;
  PA_CHECK(pa_k_flush_x(pv->m, pv->ts, T, pv->d_uu + prev, pv->d_akeep + prev, pv->buf_v[1], pv->d_X));
  pv->x_pending = 0;
  ++g_x_flushes;
  return 0;
}

/* The energy-norm drops (ecg_priv.h: energy).  Enabled between the start and the first iteration of a system solve. */
static long long g_energy_launches;
long long pa_ecg_energy_count(void) { return g_energy_launches; }
int pa_ecg_energy_enable(preAlps_ECG_t* ecg, ecg_priv_t* pv, pa_energy_t* tracker, int stop) {
  if (!tracker) return 0;
  if (ecg->bs_red != NO_BS_RED || ecg->ortho_alg == ORTHODIR_FUSED)
    return PA_FAIL("the energy-norm drops need every direction live: ORTHODIR or ORTHOMIN with NO_BS_RED");
  if (!pv->d_drop) pv->d_drop = (double*)pa_rt_malloc(PA_ENERGY_MAX_SYSTEMS * sizeof(double));
  if (!pv->h_drop) pv->h_drop = (double*)pa_rt_host_alloc_coherent(PA_ENERGY_MAX_SYSTEMS * sizeof(double));
  if (!pv->d_drop || !pv->h_drop) return PA_FAIL("no room for the energy-norm drops: %s", pa_rt_error());
  pv->energy = tracker; pv->energy_stop = stop;
  pv->poll = 0; pv->use_graphs = 0;
  return 0;
}
int pa_ecg_queue_energy(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  if (!pv->energy) return 0;
  const int k = pv->nrhs > 1 ? pv->nrhs : 1;
  PA_CHECK(pa_k_energy_drops(pv->d_alpha, ecg->alpha->info.m, ecg->alpha->info.lda, ecg->alpha->info.n, k, pv->sgrp,
                             pv->d_drop, pv->h_drop));
  ++g_energy_launches;
  return 0;
}

/* The reference's "Swapping time" (ecg.c:521-523 / :358): without block-size
 * reduction all columns are live, so the copies become pointer rotations. */
int pa_ecg_shift_directions(preAlps_ECG_t* ecg, ecg_priv_t* pv, int ncopy) {
  double t0 = pa_wtime();
  if (ecg->ortho_alg == ORTHOMIN) {
    if (pv->rotate) { double* p = pv->buf_v[0]; pv->buf_v[0] = pv->buf_z; pv->buf_z = p; }
    else PA_CHECK(pa_k_copy_cols(pv->m, pv->ts, ncopy, pv->buf_z, pv->buf_v[0]));
  } else if (pv->rotate || ncopy == ecg->enlFac) {
    /* (with block-size reduction too while every column is still live: the columns a reduction rotates away
     * stay behind in P / AP, and from then on ncopy < enlFac and the copies below keep them where they are) */
    double* oldprev = pv->buf_v[1];
    pv->buf_v[1] = pv->buf_v[0]; pv->buf_v[0] = pv->buf_z; pv->buf_z = oldprev;
    double* oldaprev = pv->buf_av[1];
    pv->buf_av[1] = pv->buf_av[0]; pv->buf_av[0] = oldaprev;
  } else {
    PA_CHECK(pa_k_copy_cols(pv->m, pv->ts, ncopy, pv->buf_v[0], pv->buf_v[1]));
    PA_CHECK(pa_k_copy_cols(pv->m, pv->ts, ncopy, pv->buf_av[0], pv->buf_av[1]));
    PA_CHECK(pa_k_copy_cols(pv->m, pv->ts, ncopy, pv->buf_z, pv->buf_v[0]));
  }
  publish_pointers(ecg, pv);
  ecg->copy_t += pa_wtime() - t0;
  return 0;
}

/* beta = AV^T Z over kbs columns of [slot 0 | slot 1] -> all-reduce ;
 * Z -= V beta (ecg.c:510-517) */
static int orthogonalise_z(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  int T = ecg->enlFac;
  int kb = ecg->beta->info.m; /* rows of beta = columns of V in use */
  int a_lo = kb < T ? kb : T, a_hi = kb - a_lo;
  double t0;
  int cnt = ecg->beta->info.lda * ecg->beta->info.n;
  const double* note = NULL;     /* device words the update kernel copies to pinned memory */
  TIC(PA_T_GRAM);
  int from_bj = pv->bj_cap > 0 ? pa_k_bj_gram_take(pv->buf_av[0], pv->buf_z) : 0;
  if (from_bj > 0 && !(a_lo == T && a_hi == T && T == 4 && ecg->beta->info.n == 4 && ecg->beta->info.lda == 8)) from_bj = 0;
  if (from_bj > 0) {
    /* the block solve left one 8 x 4 block per subdomain behind: only their sum is left to do (and, with the
     * lazy stopping test, the residual norm next to it) */
    double* scratch = pv->d_bj_parts + (size_t)pv->bj_cap * 32;
    if (pv->rtr_valid == RTR_COLUMN_SUMS && pv->lazy_ptr && pv->lazy_ptr == pv->d_beta + cnt) {
      PA_CHECK(pa_k_finish32_trace(pv->d_bj_parts, from_bj, scratch, pv->d_beta, pv->d_rtr_part, pv->rtr_nblk, pv->ts, T,
                                   pv->lazy_ptr, pv->d_info));
      pv->rtr_valid = RTR_SUMMED;
    } else {
      if (pv->rtr_valid == RTR_COLUMN_SUMS && pv->lazy_ptr) {
        PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->lazy_ptr, pv->d_info, NULL));
        pv->rtr_valid = RTR_SUMMED;
      }
      PA_CHECK(pa_k_finish32(pv->d_bj_parts, from_bj, scratch, 0, 0, pv->d_beta, NULL, NULL, NULL));
    }
  } else if (pv->rtr_valid == RTR_COLUMN_SUMS && pv->lazy_ptr && pv->lazy_ptr == pv->d_beta + cnt) {
    /* the column sums fused_first_half left: summed by the same launch, into the slot behind beta */
    PA_CHECK(pa_k_gram_finish_trace(pv->m, pv->ts, pv->buf_av[0], a_hi > 0 ? pv->buf_av[1] : NULL, pv->buf_z,
                                    pv->d_partials, a_lo, a_hi, ecg->beta->info.n, pv->d_beta, ecg->beta->info.lda,
                                    pv->d_rtr_part, pv->rtr_nblk, T, pv->lazy_ptr, pv->d_info));
    pv->rtr_valid = RTR_SUMMED;
  } else {
    if (pv->rtr_valid == RTR_COLUMN_SUMS && pv->lazy_ptr) {     /* (beta not where expected: the norm by itself) */
      PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->lazy_ptr, pv->d_info, NULL));
      pv->rtr_valid = RTR_SUMMED;
    }
    PA_CHECK(pa_k_gram_finish(pv->m, pv->ts, pv->buf_av[0], a_hi > 0 ? pv->buf_av[1] : NULL, pv->buf_z,
                              pv->d_partials, a_lo, a_hi, ecg->beta->info.n, pv->d_beta, ecg->beta->info.lda,
                              0, 0, NULL, NULL, NULL));
  }
  TAC(PA_T_GRAM, gemm_t);
  TIC(PA_T_COMM);
  {
    if (pv->rtr_valid == RTR_SUMMED && pv->lazy_ptr == pv->d_beta + cnt) {
      /* the norm of the new residual (and the Cholesky status) ride along; the update kernel
       * below passes them on to the pinned words the host reads (a copy here costs a launch and
       * 8 us of idle stream behind it);
       * several systems on several processes: their k local sums lie right behind the pair
       * (pa_k_group_norms_ride; the caller's metric: pa_k_sys_norms_ride), ride in the same collective, and reach h_grp ahead of the event below */
      if (pa_allreduce(pv->d_beta, cnt + 2 + (pa_ecg_rides(pv) ? pv->nrhs : 0))) return 1;
      if (pa_ecg_rides(pv)) PA_CHECK(pa_rt_d2h_async(pv->h_grp, pv->lazy_ptr + 2, (size_t)pv->nrhs * sizeof(double)));
      note = pv->lazy_ptr;
      pv->rtr_valid = RTR_NONE;
    } else {
      if (pa_allreduce(pv->d_beta, cnt)) return 1;
      if (pv->lazy_ptr && pv->rtr_valid == RTR_SUMMED) {   /* (beta not where expected: reduce the norm by itself) */
        if (pa_allreduce(pv->lazy_ptr, pa_ecg_rides(pv) ? 2 + pv->nrhs : 1)) return 1;
        if (pa_ecg_rides(pv)) PA_CHECK(pa_rt_d2h_async(pv->h_grp, pv->lazy_ptr + 2, (size_t)pv->nrhs * sizeof(double)));
        PA_CHECK(pa_rt_d2h_async(pv->h_pin, pv->lazy_ptr, 2 * sizeof(double)));
        PA_CHECK(pa_rt_event_record(pv->ev_res));
        pv->wait_seq = 0.0;
        pv->rtr_valid = RTR_NONE;
      }
    }
  }
  TAC(PA_T_COMM, comm_t);
  TIC(PA_T_UPDATE);
  int vn = ecg->V->info.n;
  int v_lo = vn < T ? vn : T, v_hi = vn - v_lo;
  int polled = note && pv->poll && ecg->Z->info.n > 0;
  if (polled) { pv->wait_seq = (pv->seq += 1.0); pa_k_note_seq(pv->wait_seq); }
  /* several processes: the Z written here is the X of the product that follows (shift_directions rotates it into P);
   * the rows the neighbours need are packed from the kernel's registers and the operator skips its pack launch
   * (when P turns out to be another buffer -- copies instead of rotation, BF-Omin's permuted panel -- it packs) */
  if ((g_own_loop > 0 || rci_fuse()) && pv->ts <= 4 && ecg->Z->info.n > 0 && !pv->use_graphs && pa_world_size() > 1) {
    const int* pk_off = NULL; const int* pk_slot = NULL; double* sendbuf = NULL;
    if (pa_operator_pack_hint(pv->ts, pv->buf_z, &pk_off, &pk_slot, &sendbuf) &&
        !pa_k_update_z_pack(pv->ts, pk_off, pk_slot, sendbuf))
      pa_operator_pack_hint(pv->ts, NULL, &pk_off, &pk_slot, &sendbuf);      /* (not taken: withdraw) */
  }
  PA_CHECK(pa_k_update_z(pv->m, pv->ts, v_lo, v_hi, ecg->Z->info.n, pv->d_beta, ecg->beta->info.lda,
                         pv->buf_v[0], pv->buf_v[1], pv->buf_z, note, note ? pv->h_pin : NULL,
                         pv->lazy_norm ? pv->d_uu + (size_t)pv->uu_cur * T * T : NULL,
                         pv->lazy_norm ? pv->d_uu + (size_t)(1 - pv->uu_cur) * T * T : NULL,
                         /* BF-Omin forms Z^T Z next (8 / 16 columns: the update kernel leaves its partial blocks) */
                         (ecg->ortho_alg == ORTHOMIN && ecg->bs_red == ADAPT_BS && pv->fuse) ? pv->d_partials : NULL,
                         T, &pv->zz_nblk));
  if (pv->lazy_norm) pv->uu_cur ^= 1;
  if (note && ecg->Z->info.n <= 0) PA_CHECK(pa_rt_d2h_async(pv->h_pin, note, 2 * sizeof(double)));   /* (no launch above) */
  if (note && !polled) { pv->wait_seq = 0.0; PA_CHECK(pa_rt_event_record(pv->ev_res)); }
  TAC(PA_T_UPDATE, gemm_t);
  return 0;
}

/* ---- D-Odir: reduction of the search directions (ecg.c:445-497, :593-637) -- */
static int fetch_alpha(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  PA_CHECK(pa_rt_d2h_async(pv->h_pin + 16, pv->d_alpha, (size_t)ecg->P->info.n * ecg->enlFac * sizeof(double)));
  PA_CHECK(pa_rt_event_record(pv->ev_alpha));
  return 0;
}
static int reduce_directions_odir(preAlps_ECG_t* ecg, ecg_priv_t* pv, int with_Z, int* pending_trsm, int fetched) {
  int M = ecg->globPbSize, m = pv->m, ts = pv->ts, nrhs = ecg->enlFac;
  int t = ecg->P->info.n, t1 = 0;
  double tol = ecg->tol * ecg->normb / sqrt((double)nrhs), t0;
  double* ha = pv->h_pin + 16;                 /* t x nrhs, ld t */
  double* hq = ha + (size_t)nrhs * nrhs;       /* t x t */
  double sig[16];
  t0 = pa_wtime();
  if (fetched) PA_CHECK(pa_rt_event_wait(pv->ev_alpha));     /* (fetch_alpha queued the copy; more work may be queued behind it) */
  else {
    PA_CHECK(pa_rt_d2h_async(ha, pv->d_alpha, (size_t)t * nrhs * sizeof(double)));
    PA_CHECK(pa_rt_sync());
  }
  ecg->copy_t += pa_wtime() - t0;
  t0 = pa_wtime();
  pa_sd_left_singular(t, nrhs, ha, t, hq, sig); /* hq = U, sig decreasing */
  ecg->gesvd_t += pa_wtime() - t0;
  for (int i = 0; i < t; ++i) { if (sig[i] > tol) t1++; else break; }
  if (t1 > 0 && t1 < nrhs && t1 < t) {
    t0 = pa_wtime();
    pa_sd_qr_q(t, hq);                         /* hq <- Q of the Householder QR of U */
    ecg->geqrf_t += pa_wtime() - t0;
    TIC(PA_T_UPDATE);
    pa_sd_qt_times(t, nrhs, hq, ha);           /* alpha <- Q^T alpha */
    /* keep the first t1 rows, leading dimension t1 (mkl_dimatcopy, ecg.c:483) */
    double* packed = hq + (size_t)nrhs * nrhs;
    for (int j = 0; j < nrhs; ++j) for (int i = 0; i < t1; ++i) packed[i + (size_t)t1 * j] = ha[i + (size_t)t * j];
    PA_CHECK(pa_rt_h2d(pv->d_alpha, packed, (size_t)t1 * nrhs * sizeof(double)));
    PA_CHECK(pa_rt_h2d(pv->d_q, hq, (size_t)t * t * sizeof(double)));
    if (pending_trsm && *pending_trsm) {       /* the caller held P U^-1, AP U^-1 back for its fused update */
      PA_CHECK(pa_k_trsm(m, ts, t, pv->d_mu, ecg->P->val, ecg->AP->val));
      if (pv->lazy_norm) {
        /* the panels were never normalised so far: the previous directions now, with their own factor, and the
         * block solve's result if it is already there (Z = M^-1 AP_raw: Z U^-1 is what the reference holds) */
        PA_CHECK(pa_k_trsm(m, ts, nrhs, pv->d_uu + (size_t)(1 - pv->uu_cur) * nrhs * nrhs, pv->buf_v[1], pv->buf_av[1]));
        if (pv->z_ready) PA_CHECK(pa_k_trsm(m, ts, t, pv->d_mu, ecg->Z->val, NULL));
        pv->lazy_norm = 0;
      }
      *pending_trsm = 0;
    }
    PA_CHECK(pa_k_right_mult(m, ts, t, pv->d_q, ecg->P->val));
    PA_CHECK(pa_k_right_mult(m, ts, t, pv->d_q, ecg->AP->val));
    if (with_Z || pv->z_ready) PA_CHECK(pa_k_right_mult(m, ts, t, pv->d_q, ecg->Z->val));
    TAC(PA_T_UPDATE, ormqr_t);
    CPLM_MatDenseSetInfo(ecg->alpha, t1, nrhs, t1, nrhs, COL_MAJOR);
    pa_set_desc(ecg->P, M, t1, m, t1, ts);
    pa_set_desc(ecg->AP, M, t1, m, t1, ts);
    pa_set_desc(ecg->Z, M, t1, m, t1, ts);
    ecg->bs = t1;
    ecg->kbs = t + nrhs;
  }
  CPLM_MatDenseSetInfo(ecg->beta, ecg->kbs, t1, ecg->kbs, t1, COL_MAJOR);
  pa_set_desc(ecg->V, M, ecg->kbs, m, ecg->kbs, ts);
  pa_set_desc(ecg->AV, M, ecg->kbs, m, ecg->kbs, ts);
  return 0;
}

/* ------------------------------------------------------------ Orthodir ---- */
int _preAlps_ECGIterateOdir(preAlps_ECG_t* ecg, int* rci_request) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  int t = ecg->P->info.n;
  if (*rci_request == 0) {
    if (ecg->bs_red == NO_BS_RED && pv->fuse) {
      if (fused_first_half(ecg, pv, t)) return 1;
      /* next: Z = M^-1 AP by the caller, then beta = [AP | AP_prev]^T Z here: ask the block solve for it */
      if ((g_own_loop > 0 || rci_fuse()) && pv->bj_cap > 0 && t == 4 && ecg->beta->info.m == 8 &&
          ecg->beta->info.lda == 8 && ecg->beta->info.n == 4)
        pa_k_bj_gram_arm(pv->buf_av[0], pv->buf_z, pv->buf_av[1], pv->d_bj_parts, pv->bj_cap);
      else if (pv->d_bj_parts) pa_k_bj_gram_disarm(pv->d_bj_parts);
    } else if (pv->fuse && t == ecg->enlFac) {
      /* D-Odir while every direction is still live: the same two passes, with the look at alpha in between
       * (alpha = U^-T G needs no normalised panel); a reduction decided there goes the four-pass way */
      int pending = 1;
      if (fused_gram(ecg, pv, t, 1)) return 1;
      if (fetch_alpha(ecg, pv)) return 1;
      if (g_own_loop > 0 && pv->lazy_norm) {
        if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
        pv->z_ready = 1;
      }
      if (reduce_directions_odir(ecg, pv, 0, &pending, 1)) return 1;
      if (pending ? fused_update(ecg, pv, t, NULL) : update_iterate(ecg, pv)) return 1;
    } else {
      if (a_orthonormalise_and_alpha(ecg, pv, t)) return 1;
      if (ecg->bs_red == ADAPT_BS && reduce_directions_odir(ecg, pv, 0, NULL, 0)) return 1;
      if (update_iterate(ecg, pv)) return 1;
    }
    ecg->iter++;
    *rci_request = 1;
  } else if (*rci_request == 1) {
    if (orthogonalise_z(ecg, pv)) return 1;
    if (pa_ecg_shift_directions(ecg, pv, t)) return 1;
    pa_ecg_request_gram_from_spmm(ecg, pv);
    *rci_request = 0;
  }
  return 0;
}

/* ------------------------------------------------------------ Orthomin ---- */
int _preAlps_ECGIterateOmin(preAlps_ECG_t* ecg, int* rci_request) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  int M = ecg->globPbSize, m = pv->m, ts = pv->ts, nrhs = ecg->enlFac;
  int t = ecg->P->info.n;
  if (*rci_request == 0) {
    if (pv->fuse && (ecg->bs_red == NO_BS_RED || t == nrhs)) {
      if (fused_first_half(ecg, pv, t)) return 1;   /* (BF-Omin: while the panel still has its full rank) */
    } else {
      if (a_orthonormalise_and_alpha(ecg, pv, t)) return 1;
      if (update_iterate(ecg, pv)) return 1;
    }
    ecg->iter++;
    *rci_request = 1;
  } else if (*rci_request == 1) {
    if (orthogonalise_z(ecg, pv)) return 1;
    /* BF-Omin, two passes instead of four: the copy Z -> P (ecg.c:358) waits for the pivots and is done by the
     * kernel that permutes and solves; the Gram block is formed on Z, the very numbers P would hold */
    const int one_pass = ecg->bs_red == ADAPT_BS && pv->fuse;
    if (!one_pass && pa_ecg_shift_directions(ecg, pv, nrhs)) return 1;
    if (ecg->bs_red == ADAPT_BS) {
      /* BF-Omin: G = P^T P -> pivoted Cholesky -> permute, P <- P U^-1 (ecg.c:361-393) */
      int nb = 0, rank = 0;
      double t0;
      const double* newp = one_pass ? pv->buf_z : ecg->P->val;
      TIC(PA_T_GRAM);
      if (one_pass && pv->zz_nblk > 0) nb = pv->zz_nblk;        /* (the update kernel formed the blocks of Z^T Z) */
      else PA_CHECK(pa_k_gram(m, ts, newp, NULL, newp, pv->d_partials, &nb));
      PA_CHECK(pa_k_finish(pv->d_partials, nb, 1, ts, nrhs, 0, nrhs, pv->d_mu, nrhs));
      TAC(PA_T_GRAM, gemm_t);
      TIC(PA_T_COMM);
      if (pa_allreduce(pv->d_mu, nrhs * nrhs)) return 1;
      TAC(PA_T_COMM, comm_t);
      double* hg = pv->h_pin + 16;
      PA_CHECK(pa_rt_d2h_async(hg, pv->d_mu, (size_t)nrhs * nrhs * sizeof(double)));
      PA_CHECK(pa_rt_sync());
      t0 = pa_wtime();
      pa_sd_pstrf_upper(nrhs, hg, nrhs, ecg->iwork, &rank, -1.0);
      ecg->pstrf_t += pa_wtime() - t0;
      TIC(PA_T_UPDATE);
      for (int j = 0; j < nrhs; ++j) pv->h_pin_i[j] = ecg->iwork[j] - 1;
      /* (both small copies from pinned memory without a host wait: the words are next written behind the next
       * iteration's wait for its Gram block) */
      PA_CHECK(pa_rt_h2d_async(pv->d_piv, pv->h_pin_i, nrhs * sizeof(int)));
      if (!one_pass) PA_CHECK(pa_k_permute_cols(m, ts, nrhs, pv->d_piv, ecg->P->val));
      TAC(PA_T_UPDATE, lapmt_t);
      /* leading rank x rank block, leading dimension rank for the kernel */
      double* hu = hg + (size_t)nrhs * nrhs;
      for (int j = 0; j < rank; ++j) for (int i = 0; i < rank; ++i) hu[i + (size_t)rank * j] = hg[i + (size_t)nrhs * j];
      PA_CHECK(pa_rt_h2d_async(pv->d_q, hu, (size_t)rank * rank * sizeof(double)));
      TIC(PA_T_TRSM);
      if (one_pass) {
        double tc = pa_wtime();
        PA_CHECK(pa_k_permute_trsm(m, ts, nrhs, pv->d_piv, rank, pv->d_q, pv->buf_z, pv->buf_v[0]));
        publish_pointers(ecg, pv);
        ecg->copy_t += pa_wtime() - tc;
      } else {
        PA_CHECK(pa_k_trsm(m, ts, rank, pv->d_q, ecg->P->val, NULL));
      }
      TAC(PA_T_TRSM, trsm_t);
      t = rank;
      pa_set_desc(ecg->P, M, t, m, t, ts);
      pa_set_desc(ecg->AP, M, t, m, t, ts);
      CPLM_MatDenseSetInfo(ecg->alpha, t, nrhs, t, nrhs, COL_MAJOR);
      CPLM_MatDenseSetInfo(ecg->beta, t, nrhs, t, nrhs, COL_MAJOR);
      ecg->bs = t;
    }
    pa_ecg_request_gram_from_spmm(ecg, pv);
    *rci_request = 0;
  }
  return 0;
}

/* ------------------------------------------------------ fused Orthodir ---- */
int _preAlps_ECGIterateOdirFused(preAlps_ECG_t* ecg, int* rci_request) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  int m = pv->m, ts = pv->ts, nrhs = ecg->enlFac;
  int t = ecg->P->info.n;
  double t0;
  /* the four local Gram blocks, stacked [alpha | beta | mu | RtR] (ecg.c:554-560) */
  TIC(PA_T_GRAM);
  PA_CHECK(pa_k_gram_finish(m, ts, ecg->P->val, NULL, ecg->R->val, pv->d_partials, ecg->alpha->info.m, 0,
                            ecg->alpha->info.n, pv->d_alpha, ecg->alpha->info.lda, 0, 0, NULL, NULL, NULL));
  {
    int kb = ecg->beta->info.m, a_lo = kb < nrhs ? kb : nrhs, a_hi = kb - a_lo;
    PA_CHECK(pa_k_gram_finish(m, ts, pv->buf_av[0], a_hi > 0 ? pv->buf_av[1] : NULL, pv->buf_z, pv->d_partials,
                              a_lo, a_hi, ecg->beta->info.n, pv->d_beta, ecg->beta->info.lda, 0, 0, NULL, NULL,
                              NULL));
  }
  PA_CHECK(pa_k_gram_finish(m, ts, ecg->AP->val, NULL, ecg->P->val, pv->d_partials, t, 0, t, pv->d_mu, t, 0, 0,
                            NULL, NULL, NULL));
  /* R has not changed since the previous call's update: its column norms are
   * already there, except on the first call */
  if (pv->rtr_valid == RTR_NONE) PA_CHECK(pa_k_colnorm2(m, ts, pv->d_R, pv->d_rtr_part, &pv->rtr_nblk));
  PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, ts, nrhs, pv->d_rtr, NULL, NULL));
  TAC(PA_T_GRAM, gemm_t);
  TIC(PA_T_COMM);
  if (pa_allreduce(pv->d_F, 5 * nrhs * nrhs)) return 1; /* the single reduction (ecg.c:563) */
  TAC(PA_T_COMM, comm_t);
  PA_CHECK(pa_rt_d2h_async(pv->h_pin, pv->d_rtr, sizeof(double)));
  PA_CHECK(pa_rt_sync());
  ecg->res = sqrt(pv->h_pin[0]);
  if (ecg->res < ecg->tol * ecg->normb || ecg->iter > ecg->maxIter) *rci_request = 1;
  else *rci_request = 0;
  TIC(PA_T_SMALL);
  /* mu = U^T U ; beta <- beta U^-1 ; alpha <- U^-T alpha ; beta(0:t,0:t) <- U^-T beta */
  PA_CHECK(pa_k_fused_small(pv->d_mu, t, nrhs, ecg->beta->info.m, ecg->beta->info.n, ecg->kbs,
                            pv->d_alpha, pv->d_beta, pv->d_info));
  TAC(PA_T_SMALL, potrf_t);
  TIC(PA_T_TRSM);
  PA_CHECK(pa_k_trsm(m, ts, t, pv->d_mu, ecg->P->val, ecg->AP->val));
  PA_CHECK(pa_k_trsm(m, ts, ecg->Z->info.n, pv->d_mu, ecg->Z->val, NULL));
  TAC(PA_T_TRSM, trsm_t);
  TIC(PA_T_UPDATE);
  {
    int vn = ecg->V->info.n, v_lo = vn < nrhs ? vn : nrhs, v_hi = vn - v_lo;
    PA_CHECK(pa_k_update_z(m, ts, v_lo, v_hi, ecg->Z->info.n, pv->d_beta, ecg->beta->info.lda,
                           pv->buf_v[0], pv->buf_v[1], pv->buf_z, NULL, NULL, NULL, NULL, NULL, 0, NULL));
  }
  TAC(PA_T_UPDATE, gemm_t);
  if (ecg->bs_red == ADAPT_BS && reduce_directions_odir(ecg, pv, 1, NULL, 0)) return 1;
  if (update_iterate(ecg, pv)) return 1;
  ecg->iter++;
  return pa_ecg_shift_directions(ecg, pv, ecg->bs);
}

int preAlps_ECGIterate(preAlps_ECG_t* ecg, int* rci_request) {
  double t0 = pa_wtime();
  int rc = 0;
  if (ecg->ortho_alg == ORTHOMIN) rc = _preAlps_ECGIterateOmin(ecg, rci_request);
  else if (ecg->ortho_alg == ORTHODIR) rc = _preAlps_ECGIterateOdir(ecg, rci_request);
  else if (ecg->ortho_alg == ORTHODIR_FUSED) rc = _preAlps_ECGIterateOdirFused(ecg, rci_request);
  ecg->tot_t += pa_wtime() - t0;
  return rc;
}

/* ------------------------------------------------------------ wrap up ---- */
int _preAlps_ECGWrapUp(preAlps_ECG_t* ecg, double* solution) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  if (pa_ecg_flush_x(ecg, pv)) return 1;
  /* x = X * ones (ecg.c:674); the partial sums go through the free Z buffer */
  double* d_sol = pv->d_partials;
  size_t room = pv->lay.rtr_part - pv->lay.partials;
  double* tmp = NULL;
  if ((size_t)pv->m > room) { tmp = (double*)pa_rt_malloc((size_t)pv->m * sizeof(double)); if (!tmp) return PA_FAIL("%s", pa_rt_error()); d_sol = tmp; }
  int rc = pa_k_rowsum(pv->m, pv->ts, ecg->X->info.n, pv->d_X, d_sol) ||
           pa_rt_d2h(solution, d_sol, (size_t)pv->m * sizeof(double));
  pa_rt_free(tmp);
  if (rc) return PA_FAIL("%s", pa_rt_error());
  return 0;
}

void _preAlps_ECGFree(preAlps_ECG_t* ecg) {
  ecg_priv_t* pv = priv_of(ecg);
  if (pv) {
    /* (only this object's requests: another solver's may be armed) */
    if (pv->d_spmm_parts) pa_k_spmm_gram_disarm(pv->d_spmm_parts);
    if (pv->d_bj_parts) pa_k_bj_gram_disarm(pv->d_bj_parts);
    pa_rt_sync();
    pa_rt_free(pv->d_info);
    pa_rt_free(pv->d_akeep);
    pa_rt_free(pv->d_drop);
    pa_rt_host_free(pv->h_drop);
    pa_rt_host_free(pv->h_pin);
    pa_rt_host_free(pv->h_pin_i);
    pa_rt_host_free(pv->h_grp);
    pa_rt_event_destroy(pv->ev_res);
    pa_rt_event_destroy(pv->ev_alpha);
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 6; ++b) pa_rt_graph_free(pv->graph[a][b]);
    pv->magic = 0;
  }
  free(ecg->X); free(ecg->R); free(ecg->V); free(ecg->AV); free(ecg->alpha); free(ecg->beta);
  free(ecg->Z); free(ecg->P); free(ecg->AP);
  ecg->X = ecg->R = ecg->V = ecg->AV = ecg->alpha = ecg->beta = ecg->Z = ecg->P = ecg->AP = NULL;
  pa_rt_free(ecg->work); ecg->work = NULL;
  free(ecg->iwork); ecg->iwork = NULL;
}

int preAlps_ECGFinalize(preAlps_ECG_t* ecg, double* solution) {
  ecg_priv_t* pv = priv_of(ecg);
  if (pv && pv->nrhs > 1)
    return PA_FAIL("the solver holds %d systems and one sum over the columns of X would add their solutions: "
                   "use preAlps_ECGFinalizeMulti", pv->nrhs);
  int rc = _preAlps_ECGWrapUp(ecg, solution);
  _preAlps_ECGFree(ecg);
  return rc;
}

void preAlps_ECGPrint(preAlps_ECG_t* ecg, int verbosity) {
  int rank = pa_world_rank();
  printf("[%d] prints ECG_t...\n", rank);
  printf("=== Summary ===\n");
  printf("\titer: %d\n\tres : %e\n\tbs  : %1d\n", ecg->iter, ecg->res, ecg->bs);
  printf("=== Timings ===\n");
  printf("\ttot_t  : %e s\n", ecg->tot_t);
  printf("\tcomm_t : %e s\n", ecg->comm_t);
  printf("\ttrsm_t : %e s\n", ecg->trsm_t);
  printf("\tgemm_t : %e s\n", ecg->gemm_t);
  printf("\tpotrf_t: %e s\n", ecg->potrf_t);
  printf("\tpstrf_t: %e s\n", ecg->pstrf_t);
  printf("\tlapmt_t: %e s\n", ecg->lapmt_t);
  printf("\tgesvd_t: %e s\n", ecg->gesvd_t);
  printf("\tgeqrf_t: %e s\n", ecg->geqrf_t);
  printf("\tormqr_t: %e s\n", ecg->ormqr_t);
  printf("\tcopy_t : %e s\n", ecg->copy_t);
  if (verbosity > 1 && ecg->X) {
    const char* names[9] = {"X", "R", "V", "AV", "P", "AP", "Z", "alpha", "beta"};
    CPLM_Mat_Dense_t* d[9] = {ecg->X, ecg->R, ecg->V, ecg->AV, ecg->P, ecg->AP, ecg->Z, ecg->alpha, ecg->beta};
    printf("=== Memory consumption ===\n");
    for (int i = 0; i < 9; ++i)
      printf("%s\n\tM=%d N=%d m=%d n=%d lda=%d nval=%d (HBM, %s)\n", names[i], d[i]->info.M, d[i]->info.N,
             d[i]->info.m, d[i]->info.n, d[i]->info.lda, d[i]->info.nval,
             d[i]->info.stor_type == ROW_MAJOR ? "row-interleaved" : "column major");
    printf("\n");
  }
  printf("[%d] ends printing ECG_t!\n", rank);
}
