/*
 * ecg_refine.c -- when a refined system solve stops (ecg_refine.h).  No allocation, no state, libc only.
 */
#include "ecg_refine.h"

#include <math.h>

double pa_refine_ratio(int k, const double* res, const double* thr) {
  double q = 0.0;
  for (int j = 0; j < k; ++j) {
    const double r = res[j] / thr[j];
    if (!(r >= 0.0) || isinf(r)) return INFINITY;      /* (NaN fails the comparison) */
    if (r > q) q = r;
  }
  return q;
}

int pa_refine_verdict(double q, double q_prev, int pass, int max_passes, int iters_used, int max_iter, int* keep_prev) {
  if (keep_prev) *keep_prev = 0;
  if (q <= 1.0) return PA_REFINE_CONVERGED;
  int v = PA_REFINE_CONTINUE;
  if (iters_used >= max_iter) v = PA_REFINE_OUT_OF_ITERATIONS;
  else if (pass >= 2 && (!(q <= 0.5 * q_prev) || isinf(q))) v = PA_REFINE_STAGNATED;
  else if (pass >= max_passes) v = PA_REFINE_OUT_OF_PASSES;
  /* the chain ends unconverged: the last pass may have made things worse (a pass cut short by the budget does) */
  if (v != PA_REFINE_CONTINUE && keep_prev) *keep_prev = pass >= 2 && q_prev < q;
  return v;
}

int pa_refine_passes_ok(int max_passes) { return max_passes >= 1 && max_passes <= PA_REFINE_MAX_PASSES; }
