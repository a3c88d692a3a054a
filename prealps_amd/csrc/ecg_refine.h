/*
 * ecg_refine.h -- the stop decision of preAlps_ECGSolveSystemRefined (ecg_refine.c): pure host arithmetic on libc,
 * like ecg_plan.c.  A refined solve is a chain of passes: pass 0 is preAlps_ECGSolveSystem as it is, every later pass
 * the same solve started from the x the pass before it left, whose start residual b - A x is formed with the fp64
 * values of the matrix.  Before pass p >= 1 iterates, its start residuals res[0 .. k) -- those of the x that pass
 * p - 1 left -- and the thresholds thr[j] = tol * ||b_j|| of the stopping test are known; from them, the passes and
 * the iterations spent so far, the unit says whether pass p runs.
 *
 * The measure of an iterate is its ratio q = max_j res[j] / thr[j] (q <= 1: every system meets its threshold).
 * Verdicts, the first that applies:
 *   PA_REFINE_CONVERGED          q <= 1
 *   PA_REFINE_OUT_OF_ITERATIONS  the iterations of the passes so far have used up the budget (iters_used >= max_iter)
 *   PA_REFINE_STAGNATED          p >= 2 and pass p - 1 did not halve the ratio: q > q_prev / 2, q_prev the ratio its
 *                                own start had (q == q_prev / 2 is halved)
 *   PA_REFINE_OUT_OF_PASSES      p == max_passes: every pass allowed has run
 *   PA_REFINE_CONTINUE           pass p runs, with max_iter - iters_used iterations at most
 * With the three verdicts that end the chain unconverged, *keep_prev = 1 when the iterate BEFORE pass p - 1 is the
 * better one (p >= 2 and q_prev < q: a pass that stagnated, or one that the budget cut short before it had
 * recovered from its restart), so that the caller hands back the better of the two.
 * A ratio that is not finite (NaN or Inf in a residual, a threshold of zero) never counts as converged or as halved.
 */
#ifndef PA_ECG_REFINE_H
#define PA_ECG_REFINE_H

enum {
  PA_REFINE_CONTINUE = -1,
  PA_REFINE_CONVERGED = 0,          /* (the values of `status` of preAlps_ECGSolveSystemRefined: preAlps_hip.h) */
  PA_REFINE_OUT_OF_PASSES = 1,
  PA_REFINE_OUT_OF_ITERATIONS = 2,
  PA_REFINE_STAGNATED = 3
};
#define PA_REFINE_MAX_PASSES 16

/* max_j res[j] / thr[j] over the k systems; +Inf as soon as one quotient is not a finite number >= 0 */
double pa_refine_ratio(int k, const double* res, const double* thr);

/* The verdict before pass `pass` (1 .. max_passes) iterates.  q: the ratio of its start residuals; q_prev: the ratio
 * pass - 1 started from (read only when pass >= 2); iters_used: iterations of the passes 0 .. pass - 1 together.
 * keep_prev (may be NULL) is written by every call: 1 only with a verdict that ends the chain unconverged, pass >= 2 and
 * q_prev < q. */
int pa_refine_verdict(double q, double q_prev, int pass, int max_passes, int iters_used, int max_iter, int* keep_prev);

/* 1: max_passes lies in 1 .. PA_REFINE_MAX_PASSES */
int pa_refine_passes_ok(int max_passes);

#endif
