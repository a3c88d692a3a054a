/*
 * ecg_energy.h -- the energy-norm error estimate of a block CG solve and the stopping test on it (ecg_energy.c): pure
 * host arithmetic on libc, like ecg_refine.c.  No device calls, no environment, no globals.
 *
 * With A-orthonormal directions (P^T A P = I) an iteration is X += P alpha, alpha = P^T R.  System j owns the columns
 * G_j of X and its solution is x_j = X 1_{G_j}; since P^T A E_{k+1} = 0 and R = A E column by column, one iteration
 * takes exactly
 *     delta_j(i) = || alpha_i 1_{G_j} ||_2^2
 * off the squared energy error ||x*_j - x_j||_A^2.  The norm is the same number in the caller's system and in the
 * scaled, permuted one: (D^-1 e)^T (D A D) (D^-1 e) = e^T A e.  The unit keeps every delta_j(i) of a solve
 * (cap x k doubles) and, after each push, the suffix sums
 *     D_j(l, n) = sum_{i = l}^{n - 1} delta_j(i),
 * added from the newest entry to the oldest -- never as differences of prefix sums, which cancel to exactly 0 once a
 * drop falls below eps times the running total.  D_j(l, n) is the Hestenes-Stiefel lower bound, with delay n - l, of
 * the squared error after iteration l:  e_l^2 = D_j(l, n) + e_n^2.
 *
 * The window rule (tau in (0, 0.5), dmin >= 2): l_j(n) is the largest l <= n - dmin with
 *     D_j(m, n) <= tau * D_j(l, n),   m = floor((l + n) / 2);
 * there may be none.  The estimate of the error after iteration l_j(n) is sqrt(D_j(l_j(n), n)).  Under geometric decay
 * of the drops the rule gives est^2 / true^2 >= 1 - (tau / (1 - tau))^2 (0.988 at tau = 0.1).  The estimate is a
 * HEURISTIC, not a guarantee: a fast first phase followed by a plateau can satisfy the rule while most of the error
 * is still ahead (tau = 0.25 was fooled that way on small problems; the defaults tau = 0.1, dmin = 4 are knobs, not
 * measurements).
 *
 * The stop rule: the iteration goes on while, for some system j, no l_j(n) exists or
 *     D_j(l_j(n), n) > tol^2 * D_j(0, n).
 * D_j(0, n) is a lower bound of ||x*_j - x0_j||_A^2, so the test is relative to the initial error, with or without a
 * guess.  A drop that is not a finite number >= 0 marks the tracker (pa_energy_nan) and ends the iteration.
 */
#ifndef PA_ECG_ENERGY_H
#define PA_ECG_ENERGY_H

#define PA_ENERGY_MAX_SYSTEMS 16
#define PA_ENERGY_TAU 0.1        /* the defaults of the window rule */
#define PA_ENERGY_DMIN 4

enum {
  PA_ENERGY_OK = 0,
  PA_ENERGY_BAD_ARGS = 1,        /* k, cap, tau or dmin out of range, or a NULL argument */
  PA_ENERGY_NO_MEMORY = 2,
  PA_ENERGY_FULL = 3,            /* more pushes than cap */
  PA_ENERGY_NAN = 4              /* the pushed drops hold a value that is not a finite number >= 0 (it is kept) */
};

typedef struct {
  int k, cap, n;                 /* systems, room, pushes so far */
  double tau; int dmin;
  int nan;                       /* a push was not finite or negative */
  double* delta;                 /* delta[i + j*cap] = delta_j(i) */
  double* suffix;                /* suffix[l + j*cap] = D_j(l, n) for l < n, as of the last push */
  int window[PA_ENERGY_MAX_SYSTEMS];      /* l_j(n) as of the last push, -1: none */
  int last[PA_ENERGY_MAX_SYSTEMS];        /* the l_j of the last push at which one existed, -1: never */
} pa_energy_t;

/* 1: tau lies in (0, 0.5) and dmin >= 2 (a NaN tau is out of range) */
int pa_energy_args_ok(double tau, int dmin);

/* A tracker for k systems (1 .. 16) and at most cap >= 1 pushes.  PA_ENERGY_OK, or the refusal; *e is zeroed first,
 * so pa_energy_release is safe after every outcome. */
int pa_energy_init(pa_energy_t* e, int k, int cap, double tau, int dmin);
void pa_energy_release(pa_energy_t* e);

/* The drops of one iteration, drops[j] = delta_j(n): stored, n becomes n + 1, the suffix sums and the windows are
 * formed anew.  PA_ENERGY_OK, PA_ENERGY_NAN (stored all the same; the tracker stays marked), PA_ENERGY_FULL or
 * PA_ENERGY_BAD_ARGS (nothing stored). */
int pa_energy_push(pa_energy_t* e, const double* drops);

/* D_j(l, n) of the last push, 0 <= l <= n (D_j(n, n) = 0); -1 for an index out of range */
double pa_energy_sum(const pa_energy_t* e, int j, int l);
/* l_j(n) of the last push, -1: no window qualifies */
int pa_energy_window(const pa_energy_t* e, int j);
/* 1: the iteration goes on by the stop rule above (tol: the relative tolerance, not its square); 0: every system has a
 * window whose estimate meets it -- or the tracker is marked NaN, or tol is, which stops as the residual test does */
int pa_energy_goes_on(const pa_energy_t* e, double tol);
int pa_energy_nan(const pa_energy_t* e);

/* What a solve reports at its end for system j.  L = the l_j of the last push at which a window existed:
 *   *err_iter = L (-1: none ever did), *err = sqrt(D_j(L, n)) -- the bound of the error after iteration L as the drops
 *   pushed since have sharpened it (-1 without L), *energy = sqrt(D_j(0, n));
 *   err_hist[i], i < min(n + 1, max_hist) = sqrt(D_j(i, n)) for i <= L and -1 behind it; drop_hist[i], i < min(n, max_hist)
 *   = delta_j(i).
 * Every pointer may be NULL. */
void pa_energy_report(const pa_energy_t* e, int j, double* drop_hist, double* err_hist, int max_hist, double* err,
                      int* err_iter, double* energy);

#endif
