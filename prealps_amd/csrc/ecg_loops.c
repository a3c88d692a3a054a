/*
 * ecg_loops.c -- the library's own driver loops around the RCI iteration of ecg.c: the graph segments, the
 * iteration with the block solve first, and preAlps_ECGSolve / SolveMulti / SolveGuess / SolveSystem / Advance.
 */
#include <stdlib.h>
#include <string.h>

#include "ecg_priv.h"
#include "ecg_refine.h"

/* Z = M^-1 R for Orthomin, Z = M^-1 AP otherwise */
static int apply_preconditioner(preAlps_ECG_t* ecg) {
  return preAlps_BlockJacobiApply(ecg->ortho_alg == ORTHOMIN ? ecg->R : ecg->AP, ecg->Z);
}

/* ---- graph segments ------------------------------------------------------------------------
 * seg_begin .. seg_end bracket the host code of one segment.  First pass of a (segment, phase): the
 * code runs as it is.  Second pass: the stream is captured while it runs (nothing executes), the
 * graph is instantiated and launched.  From then on the host code still runs -- it rotates
 * pointers and counts -- with every launch suppressed (pa_rt_skip), and the graph is launched in
 * its place: one launch instead of three to six per segment. */
static long long g_graph_captures, g_graph_replays;     /* segments captured / graphs launched so far, all solvers */
long long pa_ecg_graph_count(int which) { return which ? g_graph_replays : g_graph_captures; }
static int seg_begin(ecg_priv_t* pv, int seg) {
  if (!pv->use_graphs || pa_timing_enabled()) return 0;    /* (phase timers put events between the launches) */
  if (pv->bj_epoch != pa_bj_apply_epoch() || pv->op_epoch != pa_operator_plan_epoch()) {
    /* the preconditioner was created again, or its coarse space set or cleared, since the capture -- or the SpMM plan
     * was cut again, or gained or lost its fp32 copy (preAlps_hip_set_operator_precision): the graphs hold the old
     * launches and pointers (the entry that changed them has drained the stream), so capture anew */
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 6; ++b) { pa_rt_graph_free(pv->graph[a][b]); pv->graph[a][b] = NULL; pv->seen[a][b] = 0; }
    pv->bj_epoch = pa_bj_apply_epoch();
    pv->op_epoch = pa_operator_plan_epoch();
  }
  if (pv->graph[seg][pv->phase]) { pa_rt_skip(1); return 2; }
  if (pv->seen[seg][pv->phase]++ == 0) return 0;
  if (pa_rt_capture_begin()) { pv->use_graphs = 0; return 0; }   /* (nothing queued yet: go on without graphs) */
  return 1;
}
static int seg_end(ecg_priv_t* pv, int seg, int mode, int body_rc) {
  if (mode == 2) pa_rt_skip(0);
  if (mode == 1) {
    void* exec = NULL;
    int rc = pa_rt_capture_end(&exec);
    if (rc || body_rc) { pa_rt_graph_free(exec); return PA_FAIL("capturing an iteration segment failed: %s", pa_rt_error()); }
    pv->graph[seg][pv->phase] = exec;
    ++g_graph_captures;
  }
  if (body_rc) return 1;
  if (mode && pa_rt_graph_launch(pv->graph[seg][pv->phase])) return PA_FAIL("%s", pa_rt_error());
  if (mode) ++g_graph_replays;
  return 0;
}
/* One full iteration from the state "AP = A P is there" (rci 0) to the same state: the order of
 * examples/test_ecg_prealps_op.c:208-221 with the apply, the second half and the product queued
 * before the host looks at the residual norm (they do not touch X or R and are unused after a stop). */
static int graph_iteration(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* rci_request, int* stop) {
  int mode = seg_begin(pv, 0);
  int rc = preAlps_ECGIterate(ecg, rci_request) || pa_ecg_stopping_queue(ecg, pv);
  if (seg_end(pv, 0, mode, rc)) return 1;
  PA_CHECK(pa_rt_event_record(pv->ev_res));
  mode = seg_begin(pv, 1);
  rc = apply_preconditioner(ecg) || preAlps_ECGIterate(ecg, rci_request) || preAlps_BlockOperator(ecg->P, ecg->AP);
  if (seg_end(pv, 1, mode, rc)) return 1;
  pv->phase = (pv->phase + 1) % 6;
  return pa_ecg_stopping_end(ecg, pv, stop);
}

/* ---- solve first ---------------------------------------------------------------------------------------------
 * With lazy normalisation the block solve Z = M^-1 AP reads the raw AP, which the update of X and R does not touch,
 * and both Gram blocks come from raw panels: [AP | R]^T P from the SpMM, [AP | AP_prev]^T Z from the block solve.
 * So the library's own loops can run an Orthodir iteration as
 *   SpMM + Gram -> block solve + Gram -> one finish (U, alpha, beta) -> one row pass (X, R, Z and the column sums
 *   of R^2) -> the norm to the host,
 * five launches instead of six, with P read once.  Every operation and every sum is that of _preAlps_ECGIterateOdir,
 * in the same order: the results are bitwise the same.  The host must know the norm of R_k+1 before it queues the
 * row pass of the next iteration (it overwrites X and R), so the product, the block solve and the finish of that
 * iteration go out behind the norm before the host waits for it (pv->sf_ready).  After a stop they are unused: they
 * only wrote AP, Z and the Gram blocks, which a restart writes anew.  The last step of a call queues the product
 * only, as the other order does: leaving the library's loop ends the Gram request of the SpMM (pa_ecg_leave_own_loop), so
 * that order forms the first alpha of the next call with pa_k_gram_finish, and so must this one to give the same
 * bits; a call therefore returns in the state "AP = A P is queued" of the RCI protocol (rci 0), as it always did. */
static int solve_first_applies(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  return pa_ecg_in_own_loop() > 0 && ecg->P->info.n == 4 && pv->ts == 4 && !pa_ecg_rides(pv) &&      /* (several processes) */
         pa_ecg_solve_first_rule(pv->solve_first, pa_world_size(), ecg->ortho_alg, ecg->bs_red, ecg->enlFac, pv->fuse,
                                 pv->lazy_norm, pv->lazy_stop, pv->bj_cap > 0, pv->spmm_cap > 0, pv->use_graphs);
}
/* From "AP = A P is queued": the block solve and one launch that sums both Gram blocks -- U = chol(W) and alpha
 * (fused_gram) and beta (orthogonalise_z).  A product or a block solve that did not leave its block behind: the
 * block is formed here, as those two do it. */
static int sf_queue_solve(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  int m = pv->m, ts = pv->ts, t = 4, T = ecg->enlFac;
  double t0;
  pa_k_bj_gram_arm(pv->buf_av[0], pv->buf_z, pv->buf_av[1], pv->d_bj_parts, pv->bj_cap);
  if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
  int from_spmm = pa_k_spmm_gram_take(ecg->P->val, ecg->AP->val);
  int from_bj = pa_k_bj_gram_take(pv->buf_av[0], pv->buf_z);
  double* spmm_scratch = pv->d_spmm_parts + (size_t)pv->spmm_cap * 32;
  double* bj_scratch = pv->d_bj_parts + (size_t)pv->bj_cap * 32;
  TIC(PA_T_GRAM);
  if (from_spmm && from_bj) {
    PA_CHECK(pa_k_finish32_pair(pv->d_spmm_parts, from_spmm, spmm_scratch, t, T, pv->d_q, pv->d_mu, pv->d_alpha,
                                pv->d_info, pv->d_bj_parts, from_bj, bj_scratch, pv->d_beta));
  } else {
    if (from_spmm) PA_CHECK(pa_k_finish32(pv->d_spmm_parts, from_spmm, spmm_scratch, t, T, pv->d_q, pv->d_mu, pv->d_alpha,
                                         pv->d_info));
    else PA_CHECK(pa_k_gram_finish(m, ts, ecg->AP->val, pv->d_R, ecg->P->val, pv->d_partials, t, T, t, pv->d_q, t + T,
                                   t, T, pv->d_mu, pv->d_alpha, pv->d_info));
    if (from_bj) PA_CHECK(pa_k_finish32(pv->d_bj_parts, from_bj, bj_scratch, 0, 0, pv->d_beta, NULL, NULL, NULL));
    else PA_CHECK(pa_k_gram_finish(m, ts, pv->buf_av[0], pv->buf_av[1], pv->buf_z, pv->d_partials, t, t, t,
                                   pv->d_beta, 2 * t, 0, 0, NULL, NULL, NULL));
  }
  TAC(PA_T_GRAM, gemm_t);
  pv->sf_ready = 1;
  return 0;
}
/* One full iteration: the row pass, the norm to the host, the next iteration's product (ahead: and its block solve
 * and finish), then the stopping test. */
static int solve_first_step(preAlps_ECG_t* ecg, ecg_priv_t* pv, int ahead, int* stop) {
  int t = 4, T = ecg->enlFac, nb = 0;
  double tg = pa_wtime(), t0;
  if (!pv->sf_ready && sf_queue_solve(ecg, pv)) return 1;
  pv->sf_ready = 0;
  /* X moves every second pass: a pass that another one of this call follows leaves its update owed, and that one
   * applies both, in order (pa_ecg_x_mode).  What the debt needs stays put until then: P becomes the raw P_prev, U
   * is in d_uu and alpha in d_akeep (same slot), and nothing queued in between writes any of the three. */
  const int xm = pa_ecg_x_mode(pv->x_defer, pv->x_pending, ahead);
  const size_t cur = (size_t)pv->uu_cur * T * T, prev = (size_t)(1 - pv->uu_cur) * T * T;
  TIC(PA_T_UPDATE);
  PA_CHECK(pa_k_update_xrz_mode(pv->m, pv->ts, t, pv->d_mu, pv->d_alpha, ecg->P->val, ecg->AP->val, pv->buf_v[1], pv->d_X,
                                pv->d_R, pv->buf_z, pv->d_rtr_part, &nb, pv->d_uu + cur, pv->d_beta, ecg->beta->info.lda,
                                pv->d_uu + prev, xm, pv->d_akeep + (xm == PA_ECG_X_BOTH ? prev : cur)));
  TAC(PA_T_UPDATE, trsm_t);
  if (xm == PA_ECG_X_SKIP) pa_ecg_x_owed(pv);
  else pv->x_pending = 0;
  pv->rtr_nblk = nb;
  if (pa_ecg_queue_group_norms(ecg, pv, NULL)) return 1;      /* (never riding: solve_first_applies) */
  /* (d_alpha is still this iteration's: the finish of the next one is queued further down, behind the product) */
  if (pa_ecg_queue_energy(ecg, pv)) return 1;
  pv->uu_cur ^= 1;
  ecg->iter++;
  /* the norm of the new residual (and the Cholesky status) straight to the pinned words the host reads */
  pv->wait_seq = 0.0;
  if (pv->poll) { pv->wait_seq = (pv->seq += 1.0); pa_k_note_seq(pv->wait_seq); }
  PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, nb, pv->ts, T, pv->d_res2, pv->d_info, pv->h_pin));
  if (!pv->poll) PA_CHECK(pa_rt_event_record(pv->ev_res));
  pv->rtr_valid = RTR_NONE; pv->sent_seq = 0.0; pv->lazy_ptr = NULL;
  if (pa_ecg_shift_directions(ecg, pv, t)) return 1;
  pa_ecg_request_gram_from_spmm(ecg, pv);
  if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
  if (ahead && sf_queue_solve(ecg, pv)) return 1;
  ecg->tot_t += pa_wtime() - tg;
  if (pa_ecg_stopping_end(ecg, pv, stop)) return 1;
  /* a stop (tolerance, maxIter, NaN): no pass follows that would pay what this one may owe to X */
  return *stop == 1 ? pa_ecg_flush_x(ecg, pv) : 0;
}

/* one entry of the histories after a stopping test */
static void record_hist(preAlps_ECG_t* ecg, const multi_args_t* mu, double* res_hist, int* bs_hist, int max_hist,
                        int nh) {
  if (nh >= max_hist) return;
  if (res_hist) { res_hist[nh] = ecg->res; if (bs_hist) bs_hist[nh] = ecg->bs; }
  if (mu->nrhs > 0 && mu->sys_hist) {
    ecg_priv_t* pv = priv_of(ecg);
    for (int j = 0; j < mu->nrhs; ++j)
      mu->sys_hist[nh + (size_t)j * (mu->sys_hist_ld ? mu->sys_hist_ld : max_hist)] = (pv && (pv->nrhs > 1 || pv->metric)) ? pv->sys_res[j] : ecg->res;
  }
}
/* The start's norms go where the caller asked for them; *live becomes 1 when a system is above its threshold. */
static int start_norms(preAlps_ECG_t* ecg, const multi_args_t* mu, int* live) {
  double g0[16], nb[16];
  if (preAlps_ECGSystemResiduals(ecg, g0, nb)) return 1;
  for (int j = 0; j < mu->nrhs; ++j) {
    if (mu->sys_normb) mu->sys_normb[j] = nb[j];
    if (mu->sys_res0) mu->sys_res0[j] = g0[j];
    if (g0[j] > nb[j] * ecg->tol) *live = 1;
  }
  /* (a refined solve decides here whether this pass runs at all) */
  if (*live && mu->gate && mu->gate(mu->gate_ctx, mu->nrhs, g0, nb)) *live = 0;
  return 0;
}
/* The driver loop of examples/test_ecg_prealps_op.c:203-223 (fused:
 * examples/test_ecg_bench_fused.c:243-259). */
static int ecg_solve_loop(preAlps_ECG_t* ecg, double* rhs, double* sol, double* res_hist, int* bs_hist,
                          int max_hist, int* n_hist, const multi_args_t* mu) {
  int rci = 0, stop = 0, nh = 0;
  if (mu->sys) {
    int live = mu->sys->x0 == NULL;
    if (pa_ecg_start_systems("preAlps_ECGSolveSystem", ecg, mu->nrhs, NULL, 0, mu->sys->x0, mu->sys->ldx0, &rci, mu->sys)) return 1;
    if (start_norms(ecg, mu, &live)) return 1;
    if (!live) {
      /* every system meets its threshold, in the metric of the test, as it stands: x0 is the answer, bit for bit */
      if (n_hist) *n_hist = 0;
      return pa_ecg_finish_system(ecg, mu, 1);
    }
    if (pa_ecg_energy_enable(ecg, priv_of(ecg), mu->energy, mu->energy_stop)) { _preAlps_ECGFree(ecg); return 1; }
  } else if (mu->nrhs > 0 && mu->x0) {
    int live = 0;
    if (preAlps_ECGInitializeGuess(ecg, mu->nrhs, rhs, mu->ldrhs, mu->x0, mu->ldx0, &rci)) return 1;
    if (start_norms(ecg, mu, &live)) return 1;
    if (!live) {
      /* every system meets its threshold as it stands: x0 is the answer, bit for bit, and nothing is queued */
      if (n_hist) *n_hist = 0;
      if (sol) {
        const size_t m = (size_t)ecg->locPbSize;
        for (int j = 0; j < mu->nrhs; ++j)
          memcpy(sol + (size_t)j * mu->ldsol, mu->x0 + (size_t)j * mu->ldx0, m * sizeof(double));
        _preAlps_ECGFree(ecg);
      }
      return 0;
    }
  } else if (mu->nrhs > 0) {
    if (preAlps_ECGInitializeMulti(ecg, mu->nrhs, rhs, mu->ldrhs, &rci)) return 1;
    if (mu->sys_normb && preAlps_ECGSystemResiduals(ecg, NULL, mu->sys_normb)) return 1;
    if (mu->sys_res0 && preAlps_ECGSystemResiduals(ecg, NULL, mu->sys_res0)) return 1;   /* (a cold start: ||b_j||) */
  } else if (preAlps_ECGInitialize(ecg, rhs, &rci)) return 1;
  if (preAlps_BlockJacobiApply(ecg->R, ecg->P)) return 1;
  ecg_priv_t* pvg = priv_of(ecg);
  if (pvg && pvg->use_graphs) {
    if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
    while (stop != 1) {
      if (graph_iteration(ecg, pvg, &rci, &stop)) return 1;
      record_hist(ecg, mu, res_hist, bs_hist, max_hist, nh);
      ++nh;
    }
  } else if (pvg && ecg->ortho_alg != ORTHODIR_FUSED && solve_first_applies(ecg, pvg)) {
    if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
    while (stop != 1) {
      if (solve_first_step(ecg, pvg, 1, &stop)) return 1;
      record_hist(ecg, mu, res_hist, bs_hist, max_hist, nh);
      ++nh;
    }
  } else if (ecg->ortho_alg != ORTHODIR_FUSED) {
    if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
    while (stop != 1) {
      if (preAlps_ECGIterate(ecg, &rci)) return 1;
      if (rci == 0) {
        if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
      } else if (rci == 1) {
        /* same calls as the reference loop; the apply is queued before the host waits for
         * the residual norm (it does not depend on it and is simply unused after a stop) */
        ecg_priv_t* pv = priv_of(ecg);
        if (!pv) return PA_FAIL("solver not initialised");
        if (pv->z_ready) {
          /* D-Odir at full width: the first half already queued the block solve (behind which the host looked at
           * alpha); the second half and the product go out before the host waits for the norm, as below */
          pv->z_ready = 0;
          if (pa_ecg_stopping_begin(ecg, pv)) return 1;
          if (preAlps_ECGIterate(ecg, &rci)) return 1;
          if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
        } else if (pv->lazy_stop && pv->lazy_ptr) {
          /* several processes: the norm travels with the beta all-reduce of the second half;
           * the half-step and the product queued before the decision are unused after a stop */
          if (apply_preconditioner(ecg)) return 1;
          if (preAlps_ECGIterate(ecg, &rci)) return 1;
          if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
        } else {
          if (pa_ecg_stopping_begin(ecg, pv)) return 1;
          if (apply_preconditioner(ecg)) return 1;
        }
        if (pa_ecg_stopping_end(ecg, pv, &stop)) return 1;
        record_hist(ecg, mu, res_hist, bs_hist, max_hist, nh);
        ++nh;
        if (stop == 1) break;
      }
    }
  } else {
    while (rci != 1) {
      if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
      if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
      if (preAlps_ECGIterate(ecg, &rci)) return 1;
      record_hist(ecg, mu, res_hist, bs_hist, max_hist, nh);
      ++nh;
    }
  }
  if (n_hist) *n_hist = nh < max_hist ? nh : max_hist;
  if (mu->sys) return pa_ecg_finish_system(ecg, mu, 0);
  if (sol) return mu->nrhs > 0 ? preAlps_ECGFinalizeMulti(ecg, sol, mu->ldsol) : preAlps_ECGFinalize(ecg, sol);
  return 0;
}
/* ecg_solve_loop as the library's own loop (see g_own_loop in ecg.c) */
static int solve_in_own_loop(preAlps_ECG_t* ecg, double* rhs, double* sol, double* res_hist, int* bs_hist,
                             int max_hist, int* n_hist, const multi_args_t* mu) {
  pa_ecg_enter_own_loop();
  int rc = ecg_solve_loop(ecg, rhs, sol, res_hist, bs_hist, max_hist, n_hist, mu);
  ecg_priv_t* pv = priv_of(ecg);      /* (NULL where the loop has released the solver) */
  if (!rc && pv) rc = pa_ecg_flush_x(ecg, pv);
  pa_ecg_leave_own_loop();
  return rc;
}

int preAlps_ECGSolve(preAlps_ECG_t* ecg, double* rhs, double* sol, double* res_hist, int* bs_hist,
                     int max_hist, int* n_hist) {
  const multi_args_t one = {.nrhs = 0};
  return solve_in_own_loop(ecg, rhs, sol, res_hist, bs_hist, max_hist, n_hist, &one);
}
/* preAlps_ECGInitializeMulti, the loop of preAlps_ECGSolve (the same body, so the same branch of it for the same
 * settings), preAlps_ECGFinalizeMulti. */
int preAlps_ECGSolveMulti(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, double* sol, int ldsol,
                          double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                          int max_hist, int* n_hist) {
  const pa_operator_info_t* op = pa_operator_info();
  if (nrhs < 1) return PA_FAIL("nrhs = %d: at least one right-hand side is needed", nrhs);
  if (sol && op && ldsol < op->m) return PA_FAIL("ldsol = %d is smaller than the %d local rows", ldsol, op->m);
  const multi_args_t mu = {.nrhs = nrhs, .ldrhs = ldrhs, .ldsol = ldsol, .sys_hist = sys_hist, .sys_normb = sys_normb};
  return solve_in_own_loop(ecg, (double*)rhs, sol, res_hist, bs_hist, max_hist, n_hist, &mu);
}
/* The same around preAlps_ECGInitializeGuess; x0 = NULL: preAlps_ECGSolveMulti (sys_res0 then receives ||b_j||).
 * A guess under which every system already meets its threshold comes back as the solution, with no iteration. */
int preAlps_ECGSolveGuess(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, const double* x0, int ldx0,
                          double* sol, int ldsol, double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                          double* sys_res0, int max_hist, int* n_hist) {
  const pa_operator_info_t* op = pa_operator_info();
  if (nrhs < 1) return PA_FAIL("nrhs = %d: at least one right-hand side is needed", nrhs);
  if (sol && op && ldsol < op->m) return PA_FAIL("ldsol = %d is smaller than the %d local rows", ldsol, op->m);
  const multi_args_t mu = {.nrhs = nrhs, .ldrhs = ldrhs, .ldsol = ldsol, .sys_hist = sys_hist, .sys_normb = sys_normb,
                           .x0 = x0, .ldx0 = ldx0, .sys_res0 = sys_res0};
  return solve_in_own_loop(ecg, (double*)rhs, sol, res_hist, bs_hist, max_hist, n_hist, &mu);
}
/* preAlps_ECGSolveGuess around the gather and the scatter: A x = b as the caller stated it (one process: N = m; several:
 * the arrays stay global, and a rank reads and writes the rows it owns). */
/* the refusals of a system solve that its arguments alone decide; who: the entry they name */
static int system_args_refused(const char* who, const preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb,
                               const double* x0, int ldx0, const double* x, int ldx, int flags) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return pa_fail_at(who, "the operator must be built before the solver");
  if (!ecg || !b || !x) return pa_fail_at(who, " wrong test 'ecg != NULL && b != NULL && x != NULL'");
  if (nrhs < 1) return pa_fail_at(who, "nrhs = %d: at least one right-hand side is needed", nrhs);
  if (flags & ~(PREALPS_SYS_DEVICE | PREALPS_SYS_STOP_ORIGINAL)) return pa_fail_at(who, "flags = %d holds unknown bits", flags);
  /* (several processes: a leading dimension is one rank's argument, so the start takes the verdict to its agreement) */
  if (pa_world_size() > 1 || pa_comm_is_loopback()) return 0;
  if (ldb < op->N) return pa_fail_at(who, "ldb = %d is smaller than the %d rows of the matrix", ldb, op->N);
  if (x0 && ldx0 < op->N) return pa_fail_at(who, "ldx0 = %d is smaller than the %d rows of the matrix", ldx0, op->N);
  if (ldx < op->N) return pa_fail_at(who, "ldx = %d is smaller than the %d rows of the matrix", ldx, op->N);
  return 0;
}
/* sys_res0 (may be NULL): the start residuals in the metric of the test (x0 == NULL: ||b_j||); who: the entry the
 * refusals of the arguments name (solution_history.c calls this for preAlps_ECGSolveSystemHistory) */
int pa_ecg_solve_system_from(const char* who, preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, const double* x0,
                             int ldx0, double* x, int ldx, int flags, double* res_hist, int* bs_hist, double* sys_hist,
                             double* sys_normb, double* sys_res, double* sys_res0, int max_hist, int* n_hist) {
  if (system_args_refused(who, ecg, nrhs, b, ldb, x0, ldx0, x, ldx, flags)) return 1;
  const sys_in_t in = {b, ldb, x0, ldx0, (flags & PREALPS_SYS_DEVICE) != 0, (flags & PREALPS_SYS_STOP_ORIGINAL) != 0, 0, ldx};
  const multi_args_t mu = {.nrhs = nrhs, .sys_hist = sys_hist, .sys_normb = sys_normb, .sys_res0 = sys_res0, .sys = &in,
                           .sys_x = x, .sys_ldx = ldx, .sys_res = sys_res};
  return solve_in_own_loop(ecg, NULL, NULL, res_hist, bs_hist, max_hist, n_hist, &mu);
}
int preAlps_ECGSolveSystem(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, const double* x0, int ldx0, double* x,
                           int ldx, int flags, double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                           double* sys_res, int max_hist, int* n_hist) {
  return pa_ecg_solve_system_from(__func__, ecg, nrhs, b, ldb, x0, ldx0, x, ldx, flags, res_hist, bs_hist, sys_hist,
                                  sys_normb, sys_res, NULL, max_hist, n_hist);
}

/* preAlps_ECGSolveSystem with a tracker of the energy-norm drops (ecg_energy.h) that this entry owns: the loop hands it to
 * the solver behind the start (pa_ecg_energy_enable), the stopping test pushes into it, and it outlives the solver,
 * which the finish releases, so the estimates are read here. */
int preAlps_ECGSolveSystemEnergy(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, const double* x0, int ldx0,
                                 double* x, int ldx, int flags, double tau, int dmin, double* res_hist, int* bs_hist,
                                 double* sys_hist, double* sys_normb, double* sys_res, double* drop_hist, double* err_hist,
                                 double* sys_err, int* sys_err_iter, double* sys_energy, int max_hist, int* n_hist) {
  const int e_flags = PREALPS_SYS_ENERGY | PREALPS_SYS_STOP_ENERGY;
  if (!(flags & e_flags))
    return preAlps_ECGSolveSystem(ecg, nrhs, b, ldb, x0, ldx0, x, ldx, flags, res_hist, bs_hist, sys_hist, sys_normb,
                                  sys_res, max_hist, n_hist);
  if (system_args_refused(__func__, ecg, nrhs, b, ldb, x0, ldx0, x, ldx, flags & ~e_flags)) return 1;
  const int stop = (flags & PREALPS_SYS_STOP_ENERGY) != 0;
  if (stop && (flags & PREALPS_SYS_STOP_ORIGINAL))
    return pa_fail_at(__func__, "flags = %d: PREALPS_SYS_STOP_ENERGY and PREALPS_SYS_STOP_ORIGINAL are two stopping tests", flags);
  if (ecg->bs_red != NO_BS_RED || ecg->ortho_alg == ORTHODIR_FUSED)
    return pa_fail_at(__func__, "the energy-norm drops need every direction live: ORTHODIR or ORTHOMIN with NO_BS_RED, "
                                "not %s", ecg->ortho_alg == ORTHODIR_FUSED ? "ORTHODIR_FUSED" : "ADAPT_BS");
  if (!pa_energy_args_ok(tau, dmin))
    return pa_fail_at(__func__, "tau = %g, dmin = %d: tau in (0, 0.5) and dmin >= 2 are needed", tau, dmin);
  if (nrhs > PA_ENERGY_MAX_SYSTEMS) return pa_fail_at(__func__, "nrhs = %d: at most %d systems at a time", nrhs, PA_ENERGY_MAX_SYSTEMS);
  if (ecg->maxIter < 0) return pa_fail_at(__func__, "maxIter = %d", ecg->maxIter);
  pa_energy_t tr;
  /* (the loop tests after every iteration, the first included, so maxIter + 1 pushes at the most) */
  const int irc = pa_energy_init(&tr, nrhs, ecg->maxIter + 2, tau, dmin);
  if (irc) return pa_fail_at(__func__, irc == PA_ENERGY_NO_MEMORY ? "out of host memory for %d x %d drops" : "a tracker of %d x %d drops was refused", ecg->maxIter + 2, nrhs);
  const int base = flags & ~e_flags;
  const sys_in_t in = {b, ldb, x0, ldx0, (base & PREALPS_SYS_DEVICE) != 0, (base & PREALPS_SYS_STOP_ORIGINAL) != 0, 0, ldx};
  const multi_args_t mu = {.nrhs = nrhs, .sys_hist = sys_hist, .sys_normb = sys_normb, .sys = &in, .sys_x = x, .sys_ldx = ldx,
                           .sys_res = sys_res, .energy = &tr, .energy_stop = stop};
  const int rc = solve_in_own_loop(ecg, NULL, NULL, res_hist, bs_hist, max_hist, n_hist, &mu);
  ecg_priv_t* pv = priv_of(ecg);      /* (a failed solve may have left the solver standing: it must not keep the tracker) */
  if (pv) { pv->energy = NULL; pv->energy_stop = 0; }
  for (int j = 0; j < nrhs && !rc; ++j)
    pa_energy_report(&tr, j, drop_hist ? drop_hist + (size_t)j * max_hist : NULL, err_hist ? err_hist + (size_t)j * max_hist : NULL,
                     max_hist, sys_err ? sys_err + j : NULL, sys_err_iter ? sys_err_iter + j : NULL, sys_energy ? sys_energy + j : NULL);
  pa_energy_release(&tr);
  return rc;
}

/* ---- the refined system solve -----------------------------------------------------------------------------------
 * Pass 0 is preAlps_ECGSolveSystem as it is.  Every later pass p is the same solve started from the x that pass p - 1
 * left: its start forms R0 = b - A x with the fp64 values of the matrix (pa_operator_apply_exact), whatever storage
 * the iteration reads, so what a pass converged to under a rounded operator is measured, and repaired, against the
 * matrix the caller gave.  The start's norms are the verdict's input (ecg_refine.h): a start that meets every
 * threshold comes back after no iteration, as any converged guess does, and ends the chain; the gate ends it for the
 * other reasons.  The start of pass p reads a copy of x (two scratch arrays in turn, so that the iterate before the
 * last pass is still there when that pass turns out to have made things worse). */
typedef struct {
  int pass, max_passes, iters_used, max_iter, verdict, keep_prev;
  double tol, q_prev;      /* q_prev: the ratio the pass before this one started from */
} refine_gate_t;
static int refine_gate(void* ctx, int nrhs, const double* g0, const double* nb) {
  refine_gate_t* g = (refine_gate_t*)ctx;
  double thr[16];
  for (int j = 0; j < nrhs; ++j) thr[j] = nb[j] * g->tol;
  const double q = pa_refine_ratio(nrhs, g0, thr);
  g->verdict = pa_refine_verdict(q, g->q_prev, g->pass, g->max_passes, g->iters_used, g->max_iter, &g->keep_prev);
  /* (q <= 1 here, with a system a rounding above its threshold in the solver's own comparison, counts as converged) */
  if (g->verdict == PA_REFINE_CONTINUE) g->q_prev = q;
  return g->verdict != PA_REFINE_CONTINUE;
}
/* dst(:, j) = src(:, j) for the k columns of n rows, both on the device or both on the host */
static int copy_columns(int device, int n, int k, double* dst, int ldd, const double* src, int lds) {
  for (int j = 0; j < k; ++j) {
    if (!device) memcpy(dst + (size_t)j * ldd, src + (size_t)j * lds, (size_t)n * sizeof(double));
    else if (pa_rt_d2d(dst + (size_t)j * ldd, src + (size_t)j * lds, (size_t)n * sizeof(double))) return 1;
  }
  return device ? pa_rt_sync() : 0;
}
int preAlps_ECGSolveSystemRefined(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, const double* x0, int ldx0,
                                  double* x, int ldx, int flags, double* res_hist, int* bs_hist, double* sys_hist,
                                  double* sys_normb, double* sys_res, int max_hist, int* n_hist, int max_passes,
                                  int* n_passes, int* pass_iters, double* pass_res, int* status) {
  if (system_args_refused(__func__, ecg, nrhs, b, ldb, x0, ldx0, x, ldx, flags)) return 1;
  if (!pa_refine_passes_ok(max_passes))
    return PA_FAIL("max_passes = %d: between 1 and %d passes", max_passes, PA_REFINE_MAX_PASSES);
  if (nrhs > 16) return PA_FAIL("nrhs = %d: at most 16 systems at a time (what the per-system arrays of a solver hold)", nrhs);
  if (!n_passes || !pass_iters || !pass_res || !status)
    return PA_FAIL(" wrong test 'n_passes != NULL && pass_iters != NULL && pass_res != NULL && status != NULL'");
  const pa_operator_info_t* op = pa_operator_info();
  const int device = (flags & PREALPS_SYS_DEVICE) != 0, N = op->N, k = nrhs;
  const int max_iter = ecg->maxIter;
  const size_t cols = (size_t)(N > 0 ? N : 1) * k;
  double* xs[2] = {NULL, NULL};      /* the start of pass p: xs[p & 1] */
  refine_gate_t g = {.max_passes = max_passes, .max_iter = max_iter, .tol = ecg->tol};
  int nh_tot = 0, used = 0, rc = 0, p;
  double nb[16], res_end[16];
  for (int i = 0; i < (max_passes + 1) * k; ++i) pass_res[i] = 0.0;
  for (int i = 0; i < max_passes; ++i) pass_iters[i] = 0;
  *status = PA_REFINE_CONVERGED;
  for (p = 0; !rc; ++p) {      /* (left at p <= max_passes: the gate lets no pass beyond the last one run) */
    const double* start = x0;
    multi_args_t mu = {.nrhs = k, .sys_hist = sys_hist ? sys_hist + nh_tot : NULL, .sys_normb = nb, .sys_x = x, .sys_ldx = ldx,
                       .sys_res = res_end, .sys_res0 = pass_res + (size_t)p * k, .sys_hist_ld = max_hist};
    if (p > 0) {
      double** slot = &xs[p & 1];
      if (!*slot) *slot = (double*)(device ? pa_rt_malloc(cols * sizeof(double)) : malloc(cols * sizeof(double)));
      if (!*slot) { rc = PA_FAIL("no memory for the start of pass %d (%zu values)", p, cols); break; }
      if (copy_columns(device, N, k, *slot, N, x, ldx)) { rc = PA_FAIL("%s", pa_rt_error()); break; }
      start = *slot;
      g.pass = p; g.iters_used = used; g.verdict = PA_REFINE_CONVERGED;      /* (what stands when the gate is not asked) */
      mu.gate = refine_gate; mu.gate_ctx = &g;
    }
    const sys_in_t in = {b, ldb, start, p > 0 ? N : ldx0, device, (flags & PREALPS_SYS_STOP_ORIGINAL) != 0, 0, ldx};
    mu.sys = &in;
    int nh = 0;
    ecg->maxIter = max_iter - used;      /* a pass gets what is left (> 0 wherever a pass runs) */
    rc = solve_in_own_loop(ecg, NULL, NULL, res_hist ? res_hist + nh_tot : NULL, bs_hist ? bs_hist + nh_tot : NULL,
                           max_hist > nh_tot ? max_hist - nh_tot : 0, &nh, &mu);
    if (rc) break;
    if (p == 0 && sys_normb) for (int j = 0; j < k; ++j) sys_normb[j] = nb[j];
    if (sys_res) for (int j = 0; j < k; ++j) sys_res[j] = res_end[j];
    if (p > 0 && g.verdict != PA_REFINE_CONTINUE) {      /* the start ended the chain: x holds its own start again */
      *status = g.verdict;
      if (g.keep_prev) {      /* the better of the two iterates: the start of pass p - 1, and ITS residuals in sys_res */
        if (copy_columns(device, N, k, x, ldx, xs[(p - 1) & 1], N)) rc = PA_FAIL("%s", pa_rt_error());
        else if (sys_res && (flags & PREALPS_SYS_STOP_ORIGINAL))      /* (row p - 1: already in the caller's units) */
          for (int j = 0; j < k; ++j) sys_res[j] = pass_res[(size_t)(p - 1) * k + j];
        else if (sys_res) rc = preAlps_OperatorSystemResiduals(k, b, ldb, x, ldx, flags & PREALPS_SYS_DEVICE, sys_res, NULL);
      }
      break;
    }
    pass_iters[p] = ecg->iter;
    used += ecg->iter;
    nh_tot += nh;
  }
  ecg->maxIter = max_iter;
  if (!rc) {
    *n_passes = p;
    ecg->iter = used;
    if (n_hist) *n_hist = nh_tot;
  }
  if (device) { pa_rt_free(xs[0]); pa_rt_free(xs[1]); }
  else { free(xs[0]); free(xs[1]); }
  return rc;
}

/* The tail of a restart in preAlps_ECGAdvance: count it, keep what the finished solve reached, start again from the
 * same rhs up to "AP = A P is queued"; fused: Orthodir fused, whose loop queues the product itself. */
static int restart(preAlps_ECG_t* ecg, double* rhs, int* rci_request, int* restarts, int* last_iters, double* last_res,
                   int fused) {
  if (restarts) ++*restarts;
  if (last_iters) *last_iters = ecg->iter;
  if (last_res) *last_res = ecg->res;
  ecg_priv_t* pv = priv_of(ecg);
  if (pv && pa_ecg_flush_x(ecg, pv)) return 1;      /* (the stop has paid already: the reset must find nothing owed) */
  if (_preAlps_ECGReset(ecg, rhs, rci_request)) return 1;
  if (preAlps_BlockJacobiApply(ecg->R, ecg->P)) return 1;
  if (!fused && preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
  return 0;
}
/* Advance the driver loop (examples/test_ecg_prealps_op.c:208-221) by nsteps full
 * iterations, restarting from the same rhs (as after preAlps_ECGInitialize) whenever the
 * stopping test fires; what bench.py times. */
static int ecg_advance_loop(preAlps_ECG_t* ecg, double* rhs, int* rci_request, int nsteps, int* restarts,
                            int* last_iters, double* last_res) {
  int stop = 0, done = 0;
  if (ecg->ortho_alg == ORTHODIR_FUSED) {
    /* the loop of examples/test_ecg_bench_fused.c:252-259: one reduction per iteration; *rci_request
     * becomes 1 when converged (then: restart from the same rhs) */
    while (done < nsteps) {
      if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
      if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
      if (preAlps_ECGIterate(ecg, rci_request)) return 1;
      ++done;
      if (*rci_request == 1 && restart(ecg, rhs, rci_request, restarts, last_iters, last_res, 1)) return 1;
    }
    return 0;
  }
  {
    ecg_priv_t* pvg = priv_of(ecg);
    if (pvg && pvg->use_graphs && *rci_request == 0) {
      while (done < nsteps) {
        if (graph_iteration(ecg, pvg, rci_request, &stop)) return 1;
        ++done;
        if (stop == 1 && restart(ecg, rhs, rci_request, restarts, last_iters, last_res, 0)) return 1;
      }
      return 0;
    }
    if (pvg && *rci_request == 0 && solve_first_applies(ecg, pvg)) {
      while (done < nsteps) {
        if (solve_first_step(ecg, pvg, done + 1 < nsteps, &stop)) return 1;
        ++done;
        if (stop == 1 && restart(ecg, rhs, rci_request, restarts, last_iters, last_res, 0)) return 1;
      }
      return 0;
    }
  }
  while (done < nsteps) {
    if (preAlps_ECGIterate(ecg, rci_request)) return 1;
    if (*rci_request == 0) {
      if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
      ++done;
    } else {
      /* queue the stopping test, then the preconditioner apply of this iteration, and only
       * then wait for the norm: the apply does not depend on it and is discarded on stop */
      ecg_priv_t* pv = priv_of(ecg);
      if (!pv) return PA_FAIL("solver not initialised");
      int early = pv->z_ready;
      int lazy = early || (pv->lazy_stop && pv->lazy_ptr);
      if (lazy) {   /* see preAlps_ECGSolve */
        if (early) { pv->z_ready = 0; if (pa_ecg_stopping_begin(ecg, pv)) return 1; }
        else if (apply_preconditioner(ecg)) return 1;
        if (preAlps_ECGIterate(ecg, rci_request)) return 1;
        if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
      } else {
        if (pa_ecg_stopping_begin(ecg, pv)) return 1;
        if (apply_preconditioner(ecg)) return 1;
      }
      if (pa_ecg_stopping_end(ecg, pv, &stop)) return 1;
      if (lazy && stop != 1) ++done;
      if (stop == 1) {
        if (restart(ecg, rhs, rci_request, restarts, last_iters, last_res, 0)) return 1;
        ++done;
        continue;
      }
    }
  }
  return 0;
}
int preAlps_ECGAdvance(preAlps_ECG_t* ecg, double* rhs, int* rci_request, int nsteps, int* restarts,
                       int* last_iters, double* last_res) {
  ecg_priv_t* pvm = priv_of(ecg);
  if (pvm && pvm->guess)
    return PA_FAIL("the solver was started from an initial guess: a restart from the right-hand side alone would drop "
                   "x0 (use preAlps_ECGSolveGuess or the caller's own loop, or _preAlps_ECGReset for a cold start)");
  if (pvm && pvm->nrhs > 1)
    return PA_FAIL("the solver holds %d systems: restarts from one right-hand side are not defined for it "
                   "(use preAlps_ECGSolveMulti or the caller's own loop)", pvm->nrhs);
  pa_ecg_enter_own_loop();
  int rc = ecg_advance_loop(ecg, rhs, rci_request, nsteps, restarts, last_iters, last_res);
  if (!rc && pvm) rc = pa_ecg_flush_x(ecg, pvm);
  pa_ecg_leave_own_loop();
  return rc;
}
