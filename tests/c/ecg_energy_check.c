/* ecg_energy_check.c -- the energy-norm tracker (prealps_amd/csrc/ecg_energy.c) alone, as a program for the sanitizers
 * (tests/test_ecg_energy_cpu.py): ecg_energy_check <sums | rule | small | refusals | nan | report>.  Exit status 0 and
 * "ok" on the last line when every check of the mode holds; the first that does not is printed and ends the run. */
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ecg_energy.h"

#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static long double ld_sum(const double* d, int l, int n) {     /* D(l, n) in long double, newest first like the unit */
  long double s = 0.0L;
  for (int i = n - 1; i >= l; --i) s += d[i];
  return s;
}
/* l(n) by the definition, on long double sums */
static int ld_window(const double* d, int n, double tau, int dmin) {
  for (int l = n - dmin; l >= 0; --l)
    if (ld_sum(d, (l + n) / 2, n) <= (long double)tau * ld_sum(d, l, n)) return l;
  return -1;
}
static unsigned long long rng = 88172645463325252ULL;
static double uniform(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (double)(rng >> 11) / 9007199254740992.0; }

/* every D_j(l, n) after every push against long double: n - l additions, each within eps / 2 of its partial sum */
static void mode_sums(void) {
  enum { K = 3, N = 200 };
  static double d[K][N];
  pa_energy_t e;
  CHECK(pa_energy_init(&e, K, N, 0.1, 4) == PA_ENERGY_OK, "init");
  for (int i = 0; i < N; ++i) {
    double push[K];
    d[0][i] = push[0] = pow(0.8, i) * (0.5 + uniform());                   /* decay over 19 decades */
    d[1][i] = push[1] = pow(10.0, -30.0 * uniform());                      /* 30 decades, no order */
    d[2][i] = push[2] = (i % 7 == 3) ? 0.0 : uniform();                    /* zeros among O(1) */
    CHECK(pa_energy_push(&e, push) == PA_ENERGY_OK, "push %d", i);
    const int n = i + 1;
    for (int j = 0; j < K; ++j) {
      for (int l = 0; l <= n; ++l) {
        const long double want = ld_sum(d[j], l, n);
        const double got = pa_energy_sum(&e, j, l);
        CHECK(fabsl((long double)got - want) <= (long double)(n - l) * DBL_EPSILON * want, "D_%d(%d, %d) = %.17g, long double %.17Lg", j, l, n, got, want);
      }
      CHECK(pa_energy_window(&e, j) == ld_window(d[j], n, 0.1, 4), "window of system %d at n = %d: %d, by the definition %d", j, n,
            pa_energy_window(&e, j), ld_window(d[j], n, 0.1, 4));
    }
  }
  CHECK(pa_energy_sum(&e, 0, N + 1) == -1.0 && pa_energy_sum(&e, K, 0) == -1.0 && pa_energy_sum(&e, 0, -1) == -1.0, "out of range");
  pa_energy_release(&e);
}

static void mode_rule(void) {
  pa_energy_t e;
  /* geometric decay delta_i = q^i: the true squared error after l iterations is q^l / (1 - q); wherever a window
   * exists, est^2 / true^2 >= 1 - (tau / (1 - tau))^2 (the model bound), and the stop rule fires once est meets tol */
  const double qs[3] = {0.5, 0.8, 0.95}, taus[2] = {0.1, 0.25};
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 2; ++b) {
    const double q = qs[a], tau = taus[b], model = 1.0 - (tau / (1.0 - tau)) * (tau / (1.0 - tau));
    CHECK(pa_energy_init(&e, 1, 600, tau, 4) == PA_ENERGY_OK, "init");
    int first = -1, stopped = -1;
    for (int i = 0; i < 600; ++i) {
      const double drop = pow(q, i);
      CHECK(pa_energy_push(&e, &drop) == PA_ENERGY_OK, "push");
      const int n = i + 1, l = pa_energy_window(&e, 0);
      if (l >= 0) {
        if (first < 0) first = n;
        CHECK(l <= n - 4, "l = %d at n = %d", l, n);
        const double est2 = pa_energy_sum(&e, 0, l), true2 = pow(q, l) / (1.0 - q);
        CHECK(est2 <= true2 * (1.0 + 1e-12), "a lower bound: est^2 %.17g, true^2 %.17g", est2, true2);
        CHECK(est2 >= model * true2 * (1.0 - 1e-12), "q = %g tau = %g n = %d l = %d: est^2 / true^2 = %.6f under the model's %.6f", q, tau, n, l, est2 / true2, model);
      } else CHECK(first < 0, "q = %g: a window at n = %d and none at %d", q, first, n);
      const int on = pa_energy_goes_on(&e, 1e-3);
      if (l < 0) CHECK(on == 1, "no window: the iteration goes on");
      else CHECK(on == (pa_energy_sum(&e, 0, l) > 1e-6 * pa_energy_sum(&e, 0, 0)), "the stop rule at n = %d", n);
      if (!on && stopped < 0) stopped = n;
    }
    CHECK(first > 0 && stopped > first, "q = %g tau = %g: first window at %d, stop at %d", q, tau, first, stopped);
    printf("geometric q = %g tau = %g: first window at n = %d, stop (tol 1e-3) at n = %d\n", q, tau, first, stopped);
    pa_energy_release(&e);
  }
  /* a fast first phase, then a plateau: windows inside the plateau hold half their sum in the second half, so only
   * l in the first phase can qualify, whose estimate is that of the START's error: the rule must go on */
  CHECK(pa_energy_init(&e, 1, 100, 0.1, 4) == PA_ENERGY_OK, "init");
  for (int i = 0; i < 100; ++i) {
    const double drop = i < 3 ? pow(1e-2, i) : 1e-6;
    CHECK(pa_energy_push(&e, &drop) == PA_ENERGY_OK, "push");
    const int l = pa_energy_window(&e, 0);
    CHECK(l <= 2, "plateau: window %d at n = %d lies in the plateau", l, i + 1);
    CHECK(pa_energy_goes_on(&e, 5e-3) == 1, "plateau: stopped at n = %d with window %d", i + 1, l);
  }
  pa_energy_release(&e);
  /* one small drop between large ones: no window ever qualifies */
  CHECK(pa_energy_init(&e, 2, 40, 0.1, 4) == PA_ENERGY_OK, "init");
  for (int i = 0; i < 40; ++i) {
    const double drop[2] = {i == 3 ? 1e-12 : 1.0, i == 20 ? 0.0 : 2.0};
    CHECK(pa_energy_push(&e, drop) == PA_ENERGY_OK, "push");
    CHECK(pa_energy_window(&e, 0) == -1 && pa_energy_window(&e, 1) == -1, "a window at n = %d: %d %d", i + 1, pa_energy_window(&e, 0), pa_energy_window(&e, 1));
    CHECK(pa_energy_goes_on(&e, 0.5) == 1, "stopped at n = %d", i + 1);
  }
  pa_energy_release(&e);
  /* two systems: the slower one holds the stop back */
  CHECK(pa_energy_init(&e, 2, 200, 0.1, 4) == PA_ENERGY_OK, "init");
  int stop0 = -1, stop_both = -1;
  for (int i = 0; i < 200; ++i) {
    const double drop[2] = {pow(0.3, i), pow(0.8, i)};
    CHECK(pa_energy_push(&e, drop) == PA_ENERGY_OK, "push");
    const int l0 = pa_energy_window(&e, 0);
    if (stop0 < 0 && l0 >= 0 && pa_energy_sum(&e, 0, l0) <= 1e-8 * pa_energy_sum(&e, 0, 0)) stop0 = i + 1;
    if (stop_both < 0 && !pa_energy_goes_on(&e, 1e-4)) stop_both = i + 1;
  }
  CHECK(stop0 > 0 && stop_both > stop0 + 10, "system 0 alone at %d, both at %d", stop0, stop_both);
  pa_energy_release(&e);
}

/* drops below eps times the running total: a difference of prefix sums gives exactly 0, the suffix sums do not */
static void mode_small(void) {
  enum { N = 40 };
  double d[N], prefix[N + 1];
  pa_energy_t e;
  CHECK(pa_energy_init(&e, 1, N, 0.1, 4) == PA_ENERGY_OK, "init");
  prefix[0] = 0.0;
  for (int i = 0; i < N; ++i) {
    d[i] = i == 0 ? 1.0 : 1e-20 * pow(0.5, i);
    prefix[i + 1] = prefix[i] + d[i];
    CHECK(pa_energy_push(&e, &d[i]) == PA_ENERGY_OK, "push");
  }
  CHECK(prefix[N] - prefix[1] == 0.0, "the case is the one meant: prefix sums cancel");
  for (int l = 1; l < N; ++l) {
    const double got = pa_energy_sum(&e, 0, l);
    const long double want = ld_sum(d, l, N);
    CHECK(got > 0.0 && fabsl((long double)got - want) <= (long double)(N - l) * DBL_EPSILON * want, "D(%d, %d) = %.17g, long double %.17Lg", l, N, got, want);
  }
  /* and the rule sees the decay of the small drops: a window behind the first entry, whose estimate meets 1e-9 */
  CHECK(pa_energy_window(&e, 0) >= 1, "window %d", pa_energy_window(&e, 0));
  CHECK(pa_energy_goes_on(&e, 1e-9) == 0 && pa_energy_goes_on(&e, 1e-16) == 1, "the stop rule on the small drops");
  pa_energy_release(&e);
}

static void mode_refusals(void) {
  pa_energy_t e;
  const double one = 1.0;
  CHECK(pa_energy_args_ok(0.1, 4) && pa_energy_args_ok(0.49, 2) && pa_energy_args_ok(1e-300, 1000), "accepted");
  CHECK(!pa_energy_args_ok(0.0, 4) && !pa_energy_args_ok(0.5, 4) && !pa_energy_args_ok(-0.1, 4) && !pa_energy_args_ok(NAN, 4) &&
        !pa_energy_args_ok(INFINITY, 4) && !pa_energy_args_ok(0.1, 1) && !pa_energy_args_ok(0.1, 0) && !pa_energy_args_ok(0.1, -3), "refused");
  CHECK(pa_energy_init(NULL, 1, 10, 0.1, 4) == PA_ENERGY_BAD_ARGS, "NULL");
  CHECK(pa_energy_init(&e, 0, 10, 0.1, 4) == PA_ENERGY_BAD_ARGS && e.delta == NULL, "k = 0");
  CHECK(pa_energy_init(&e, 17, 10, 0.1, 4) == PA_ENERGY_BAD_ARGS, "k = 17");
  CHECK(pa_energy_init(&e, 1, 0, 0.1, 4) == PA_ENERGY_BAD_ARGS, "cap = 0");
  CHECK(pa_energy_init(&e, 1, 10, 0.5, 4) == PA_ENERGY_BAD_ARGS, "tau = 0.5");
  CHECK(pa_energy_init(&e, 1, 10, 0.1, 1) == PA_ENERGY_BAD_ARGS, "dmin = 1");
  pa_energy_release(&e);                                   /* (safe behind a refusal) */
  CHECK(pa_energy_push(&e, &one) == PA_ENERGY_BAD_ARGS, "a push into a tracker that was refused");
  CHECK(pa_energy_goes_on(&e, 1e-5) == 0 && pa_energy_window(&e, 0) == -1 && pa_energy_sum(&e, 0, 0) == -1.0, "an empty tracker");
  CHECK(pa_energy_init(&e, 16, 3, 0.1, 2) == PA_ENERGY_OK, "16 systems");
  double drops[16];
  for (int j = 0; j < 16; ++j) drops[j] = j + 1.0;
  CHECK(pa_energy_push(&e, NULL) == PA_ENERGY_BAD_ARGS && e.n == 0, "NULL drops");
  CHECK(pa_energy_goes_on(&e, 1e-5) == 1, "before the first push no window exists");
  for (int i = 0; i < 3; ++i) CHECK(pa_energy_push(&e, drops) == PA_ENERGY_OK, "push %d", i);
  CHECK(pa_energy_push(&e, drops) == PA_ENERGY_FULL && e.n == 3, "a fourth push into room for three");
  CHECK(pa_energy_sum(&e, 15, 0) == 48.0 && pa_energy_sum(&e, 15, 3) == 0.0, "the sums of system 15");
  pa_energy_release(&e);
  pa_energy_release(&e);
  pa_energy_release(NULL);
}

static void mode_nan(void) {
  const double bad[4] = {NAN, INFINITY, -1.0, -INFINITY};
  for (int b = 0; b < 4; ++b) {
    pa_energy_t e;
    CHECK(pa_energy_init(&e, 2, 50, 0.1, 4) == PA_ENERGY_OK, "init");
    for (int i = 0; i < 30; ++i) {
      const double drop[2] = {pow(0.2, i), i == 12 ? bad[b] : pow(0.3, i)};
      const int rc = pa_energy_push(&e, drop);
      CHECK(rc == (i == 12 ? PA_ENERGY_NAN : PA_ENERGY_OK), "push %d returned %d", i, rc);
      CHECK(pa_energy_nan(&e) == (i >= 12), "the mark at push %d", i);
      if (i >= 12) CHECK(pa_energy_goes_on(&e, 1e-30) == 0, "a marked tracker stops (push %d)", i);
    }
    CHECK(e.n == 30, "the drops are kept");
    pa_energy_release(&e);
  }
  pa_energy_t e;
  const double one = 1.0;
  CHECK(pa_energy_init(&e, 1, 5, 0.1, 2) == PA_ENERGY_OK && pa_energy_push(&e, &one) == PA_ENERGY_OK, "init");
  CHECK(pa_energy_goes_on(&e, NAN) == 0, "a NaN tolerance stops");
  pa_energy_release(&e);
}

static void mode_report(void) {
  enum { N = 30, MH = 40 };
  pa_energy_t e;
  double d[N], drop_hist[MH], err_hist[MH], err, energy;
  int it;
  CHECK(pa_energy_init(&e, 2, N, 0.1, 4) == PA_ENERGY_OK, "init");
  for (int i = 0; i < N; ++i) {
    const double drop[2] = {d[i] = pow(0.4, i), 1.0};
    CHECK(pa_energy_push(&e, drop) == PA_ENERGY_OK, "push");
  }
  for (int i = 0; i < MH; ++i) drop_hist[i] = err_hist[i] = 77.0;
  pa_energy_report(&e, 0, drop_hist, err_hist, MH, &err, &it, &energy);
  CHECK(it == pa_energy_window(&e, 0) && it >= 20 && it <= N - 4, "err_iter %d", it);
  CHECK(err == sqrt(pa_energy_sum(&e, 0, it)) && energy == sqrt(pa_energy_sum(&e, 0, 0)), "err, energy");
  for (int i = 0; i < MH; ++i) {
    CHECK(drop_hist[i] == (i < N ? d[i] : 77.0), "drop_hist[%d]", i);
    CHECK(err_hist[i] == (i <= it ? sqrt(pa_energy_sum(&e, 0, i)) : i <= N ? -1.0 : 77.0), "err_hist[%d] = %g", i, err_hist[i]);
  }
  for (int i = 0; i < MH; ++i) err_hist[i] = 77.0;
  pa_energy_report(&e, 1, NULL, err_hist, 5, &err, &it, &energy);      /* equal drops: no window, ever; a short history */
  CHECK(it == -1 && err == -1.0 && energy == sqrt((double)N), "system 1: %d %g %g", it, err, energy);
  for (int i = 0; i < MH; ++i) CHECK(err_hist[i] == (i < 5 ? -1.0 : 77.0), "err_hist[%d]", i);
  pa_energy_report(&e, 0, NULL, NULL, 0, NULL, NULL, NULL);
  pa_energy_release(&e);
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "sums")) mode_sums();
  else if (!strcmp(mode, "rule")) mode_rule();
  else if (!strcmp(mode, "small")) mode_small();
  else if (!strcmp(mode, "refusals")) mode_refusals();
  else if (!strcmp(mode, "nan")) mode_nan();
  else if (!strcmp(mode, "report")) mode_report();
  else { printf("usage: ecg_energy_check <sums | rule | small | refusals | nan | report>\n"); return 2; }
  printf("ok\n");
  return 0;
}
