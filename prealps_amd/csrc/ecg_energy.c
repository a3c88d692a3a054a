/*
 * ecg_energy.c -- the energy-norm drops of a block CG solve, their suffix sums, the window rule and the stopping test
 * on it (see ecg_energy.h for the identity, the rule and its limits).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ecg_energy.h"

int pa_energy_args_ok(double tau, int dmin) { return tau > 0.0 && tau < 0.5 && dmin >= 2; }

int pa_energy_init(pa_energy_t* e, int k, int cap, double tau, int dmin) {
  if (!e) return PA_ENERGY_BAD_ARGS;
  memset(e, 0, sizeof(*e));
  if (k < 1 || k > PA_ENERGY_MAX_SYSTEMS || cap < 1 || !pa_energy_args_ok(tau, dmin)) return PA_ENERGY_BAD_ARGS;
  e->delta = (double*)calloc((size_t)cap * k, sizeof(double));
  e->suffix = (double*)calloc((size_t)cap * k, sizeof(double));
  if (!e->delta || !e->suffix) { pa_energy_release(e); return PA_ENERGY_NO_MEMORY; }
  e->k = k; e->cap = cap; e->tau = tau; e->dmin = dmin;
  for (int j = 0; j < PA_ENERGY_MAX_SYSTEMS; ++j) e->window[j] = e->last[j] = -1;
  return PA_ENERGY_OK;
}

void pa_energy_release(pa_energy_t* e) {
  if (!e) return;
  free(e->delta);
  free(e->suffix);
  memset(e, 0, sizeof(*e));
}

int pa_energy_push(pa_energy_t* e, const double* drops) {
  if (!e || !e->delta || !drops) return PA_ENERGY_BAD_ARGS;
  if (e->n >= e->cap) return PA_ENERGY_FULL;
  int bad = 0;
  const int n = e->n + 1;
  for (int j = 0; j < e->k; ++j) {
    const double d = drops[j];
    double* dj = e->delta + (size_t)j * e->cap;
    double* sj = e->suffix + (size_t)j * e->cap;
    if (!(d >= 0.0) || !(d - d == 0.0)) bad = 1;
    dj[n - 1] = d;
    /* from the newest entry to the oldest: the small recent drops are summed before the large old ones join them, so
     * none of them is lost, and D_j(l, n) with l near n never comes out as a cancelled difference */
    double run = 0.0;
    for (int l = n - 1; l >= 0; --l) { run += dj[l]; sj[l] = run; }
    /* the largest l <= n - dmin whose second half holds at most tau of the whole window */
    int w = -1;
    for (int l = n - e->dmin; l >= 0; --l) {
      const int m = (l + n) / 2;
      if (sj[m] <= e->tau * sj[l]) { w = l; break; }
    }
    e->window[j] = w;
    if (w >= 0) e->last[j] = w;
  }
  e->n = n;
  if (bad) e->nan = 1;
  return bad ? PA_ENERGY_NAN : PA_ENERGY_OK;
}

double pa_energy_sum(const pa_energy_t* e, int j, int l) {
  if (!e || !e->suffix || j < 0 || j >= e->k || l < 0 || l > e->n) return -1.0;
  return l == e->n ? 0.0 : e->suffix[l + (size_t)j * e->cap];
}

int pa_energy_window(const pa_energy_t* e, int j) {
  if (!e || j < 0 || j >= e->k) return -1;
  return e->window[j];
}

int pa_energy_nan(const pa_energy_t* e) { return e ? e->nan : 0; }

int pa_energy_goes_on(const pa_energy_t* e, double tol) {
  if (!e || !e->suffix || e->nan || !(tol == tol)) return 0;
  for (int j = 0; j < e->k; ++j) {
    const int l = e->window[j];
    if (l < 0) return 1;
    const double* sj = e->suffix + (size_t)j * e->cap;
    if (sj[l] > tol * tol * sj[0]) return 1;
  }
  return 0;
}

void pa_energy_report(const pa_energy_t* e, int j, double* drop_hist, double* err_hist, int max_hist, double* err,
                      int* err_iter, double* energy) {
  const int ok = e && e->suffix && j >= 0 && j < e->k;
  const int n = ok ? e->n : 0, L = ok ? e->last[j] : -1;
  if (err_iter) *err_iter = L;
  if (err) *err = L >= 0 ? sqrt(pa_energy_sum(e, j, L)) : -1.0;
  if (energy) *energy = ok ? sqrt(pa_energy_sum(e, j, 0)) : 0.0;
  for (int i = 0; drop_hist && i < n && i < max_hist; ++i) drop_hist[i] = e->delta[i + (size_t)j * e->cap];
  for (int i = 0; err_hist && i <= n && i < max_hist; ++i) err_hist[i] = i <= L ? sqrt(pa_energy_sum(e, j, i)) : -1.0;
}
