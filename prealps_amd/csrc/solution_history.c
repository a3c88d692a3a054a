/*
 * solution_history.c -- the solution history of the built operator (preAlps_SolutionHistory*, preAlps_ECGSolveSystemHistory):
 * the device ring Xh of the last solutions in the caller's order and units, the glue around the host unit
 * ecg_history.c (ring, Gram matrix, pivoted Cholesky) and the kernels of history.hip (dots, combine).
 *   w = A x is the library's own fp64 product, formed as preAlps_OperatorSystemResiduals forms it: a temporary solver
 * of width q at s = 1, pa_k_sys_gather for (D^-1 x)[perm], pa_k_guess_split into its X panel and
 * pa_operator_apply_exact into its Z panel; the mapped dots read that panel through the operator's row map, so
 * x_i^T (A x_j) comes out in the caller's units, where it is the same number as in the scaled, permuted system.
 *   One process only: the dots would need an all-reduce and the product the halo exchange.  Every entry drains the
 * library stream before it returns, as the set-up entries do.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "ecg_priv.h"
#include "ecg_history.h"

typedef struct {
  int live;
  pa_hist_t h;
  int N, build;            /* rows of the operator the ring was cut for, and pa_operator_build_count() then */
  int epoch;               /* pa_operator_values_epoch() G was formed at */
  double* d_X;             /* N x cap, column major, ld N */
  double* d_part;          /* the partial sums of a dots launch */
  double* d_small;         /* [0, 256): the K x q block of a dots launch, [256, 512): the coefficients */
  long long appends, projections, refreshes;
  int last_rank;
} history_t;
static history_t g_hist;

#define FAIL_AS(who, ...) pa_fail_at(who, __VA_ARGS__)

int preAlps_SolutionHistoryFree(void) {
  if (g_hist.live) { pa_rt_sync(); pa_rt_free(g_hist.d_X); pa_rt_free(g_hist.d_part); pa_rt_free(g_hist.d_small); }
  memset(&g_hist, 0, sizeof(g_hist));
  return 0;
}

/* 0: key is one of the history's and *value is written (all 0 without a history) */
int pa_hist_stat(const char* key, double* value) {
  const history_t* g = &g_hist;
  if (!strcmp(key, "hist_capacity")) *value = g->live ? g->h.cap : 0;
  else if (!strcmp(key, "hist_columns")) *value = g->live ? g->h.count : 0;
  else if (!strcmp(key, "hist_bytes")) *value = g->live ? 8.0 * (double)g->N * g->h.cap : 0.0;
  else if (!strcmp(key, "hist_appends")) *value = (double)g->appends;
  else if (!strcmp(key, "hist_projections")) *value = (double)g->projections;
  else if (!strcmp(key, "hist_last_rank")) *value = g->last_rank;
  else if (!strcmp(key, "hist_gram_refreshes")) *value = (double)g->refreshes;
  else if (!strcmp(key, "hist_values_epoch")) *value = g->live ? g->epoch : 0;
  else return 1;
  return 0;
}

/* what every entry refuses before it looks at its arrays; need_hist: a history must exist */
static int refused(const char* who, int need_hist) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return FAIL_AS(who, "the operator must be built first");
  if (pa_operator_plan_only()) return FAIL_AS(who, "the operator was built in plan-only mode (no GPU)");
  if (pa_world_size() > 1 || pa_comm_is_loopback())
    return FAIL_AS(who, "a solution history needs a single process (%d processes%s): its dots are not reduced",
                   pa_world_size(), pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "");
  if (need_hist && g_hist.live && (g_hist.build != pa_operator_build_count() || g_hist.N != op->N))
    preAlps_SolutionHistoryFree();      /* (the operator it belonged to is gone) */
  if (need_hist && !g_hist.live) return FAIL_AS(who, "no solution history (preAlps_SolutionHistoryCreate)");
  return 0;
}
static int array_refused(const char* who, const pa_operator_info_t* op, int nrhs, const void* a, int ld, const char* name) {
  if (nrhs < 1 || nrhs > PA_HIST_MAX) return FAIL_AS(who, "nrhs = %d: between 1 and %d columns at a time", nrhs, PA_HIST_MAX);
  if (!a) return FAIL_AS(who, " wrong test '%s != NULL'", name);
  if (ld < op->N) return FAIL_AS(who, "ld%s = %d is smaller than the %d rows of the matrix", name, ld, op->N);
  return 0;
}

int preAlps_SolutionHistoryCreate(int capacity) {
  if (refused(__func__, 0)) return 1;
  if (!pa_hist_capacity_ok(capacity)) return PA_FAIL("capacity = %d: between 1 and %d solutions", capacity, PA_HIST_MAX);
  PA_REQUIRE_GPU();
  const pa_operator_info_t* op = pa_operator_info();
  history_t n;
  memset(&n, 0, sizeof(n));
  const size_t nn = (size_t)(op->N > 0 ? op->N : 1);
  n.d_X = (double*)pa_rt_malloc(nn * capacity * sizeof(double));
  n.d_part = (double*)pa_rt_malloc(pa_k_hist_part_doubles() * sizeof(double));
  n.d_small = (double*)pa_rt_malloc(512 * sizeof(double));
  if (!n.d_X || !n.d_part || !n.d_small) {
    pa_rt_free(n.d_X); pa_rt_free(n.d_part); pa_rt_free(n.d_small);
    return PA_FAIL("%d columns of %d rows on the device: %s", capacity, op->N, pa_rt_error());
  }
  preAlps_SolutionHistoryFree();
  pa_hist_init(&n.h, capacity);
  n.live = 1; n.N = op->N; n.build = pa_operator_build_count(); n.epoch = pa_operator_values_epoch();
  g_hist = n;
  return 0;
}

int preAlps_SolutionHistoryClear(void) {
  if (refused(__func__, 1)) return 1;
  PA_CHECK(pa_rt_sync());
  pa_hist_clear(&g_hist.h);
  g_hist.epoch = pa_operator_values_epoch();
  return 0;
}

/* a caller's array on the device: itself, or a copy of its q columns (ld N) in *tmp */
static int on_device(const char* who, const double* a, int ld, int q, int device, double** tmp, const double** d, int* ldd) {
  const int N = g_hist.N;
  *tmp = NULL;
  if (device) { *d = a; *ldd = ld; return 0; }
  *tmp = (double*)pa_rt_malloc((size_t)(N > 0 ? N : 1) * q * sizeof(double));
  if (!*tmp) return FAIL_AS(who, "%d columns on the device: %s", q, pa_rt_error());
  for (int j = 0; j < q; ++j)
    if (pa_rt_h2d(*tmp + (size_t)j * N, a + (size_t)j * ld, (size_t)N * sizeof(double))) {
      pa_rt_free(*tmp); *tmp = NULL;
      return FAIL_AS(who, "%s", pa_rt_error());
    }
  *d = *tmp; *ldd = N;
  return 0;
}

/* W' = A' (D^-1 x)[perm] for the q columns of d_x (device, the caller's order and units) in the Z panel of the
 * temporary solver e, which the caller releases (_preAlps_ECGFree) whatever this returns */
static int product(const char* who, int q, const double* d_x, int ldx, preAlps_ECG_t* e, const int** src, const double** dl) {
  const pa_operator_info_t* op = pa_operator_info();
  const int m = op->m;
  memset(e, 0, sizeof(*e));
  /* at the width the SpMM plan in use was cut for, where the columns fit it: a narrower panel would cut the plan
   * again here and once more at the next solve (the columns beyond q stay zero) */
  const int pts = pa_operator_plan_stride();
  e->globPbSize = op->N; e->locPbSize = m; e->enlFac = (pts >= q && pts <= 16) ? pts : q; e->maxIter = 1; e->tol = 1e-5;
  e->ortho_alg = ORTHODIR; e->bs_red = NO_BS_RED;
  if (_preAlps_ECGMalloc(e)) return 1;
  ecg_priv_t* pv = priv_of(e);
  if (pa_ecg_reset_state(e, pv, q, 1, 0)) return 1;
  if (pa_operator_system_map(src, dl)) return 1;
  const size_t mm = (size_t)(m > 0 ? m : 1);
  double* st = (double*)pa_rt_malloc(2 * mm * q * sizeof(double) + mm * sizeof(int));
  if (!st) return FAIL_AS(who, "staging %d columns: %s", q, pa_rt_error());
  int* d_pcol = (int*)(st + 2 * mm * q);
  int gblk = 0;
  /* s = 1: every row puts its entry into column j of system j (pcol = 0); the gather's copy of d * x is not used */
  int rc = pa_rt_memset(d_pcol, 0, mm * sizeof(int)) ||
           pa_k_sys_gather(m, pv->ts, q, *src, *dl, d_x, ldx, d_x, ldx, st, st + mm * q, pv->d_sys_part, &gblk) ||
           pa_k_guess_split(m, pv->ts, q, 1, st + mm * q, m, d_pcol, pv->d_X);
  if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  if (!rc) rc = pa_operator_apply_exact(e->X, e->Z);
  if (pa_rt_sync() && !rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  pa_rt_free(st);
  return rc;
}

/* G again from Xh and the matrix as it is now, when the values have moved since G was formed */
static int refresh(const char* who) {
  history_t* g = &g_hist;
  const int now = pa_operator_values_epoch();
  if (g->epoch == now) return 0;
  if (g->h.count == 0) { g->epoch = now; return 0; }
  const int K = g->h.count;
  preAlps_ECG_t e;
  const int* src; const double* dl;
  double D[PA_HIST_MAX * PA_HIST_MAX];
  int rc = product(who, K, g->d_X, g->N, &e, &src, &dl);
  ecg_priv_t* pv = priv_of(&e);
  if (!rc && (pa_k_hist_dots_mapped(pa_operator_info()->m, K, K, g->d_X, g->N, 0, K, src, dl, pv->buf_z, pv->ts, g->d_part, g->d_small) ||
              pa_rt_d2h(D, g->d_small, (size_t)K * K * sizeof(double))))
    rc = FAIL_AS(who, "%s", pa_rt_error());
  _preAlps_ECGFree(&e);
  if (rc) return 1;
  pa_hist_set_gram(&g->h, D, K);
  g->epoch = now;
  ++g->refreshes;
  return 0;
}

static int append(const char* who, int nrhs, const double* x, int ldx, int device) {
  history_t* g = &g_hist;
  if (refresh(who)) return 1;
  const int K = g->h.count, q = nrhs, m = pa_operator_info()->m;
  double* tmp; const double* d_x; int ldd;
  if (on_device(who, x, ldx, q, device, &tmp, &d_x, &ldd)) return 1;
  preAlps_ECG_t e;
  const int* src; const double* dl;
  double DO[PA_HIST_MAX * PA_HIST_MAX], DN[PA_HIST_MAX * PA_HIST_MAX];
  int slots[PA_HIST_MAX];
  int rc = product(who, q, d_x, ldd, &e, &src, &dl);
  ecg_priv_t* pv = priv_of(&e);
  if (!rc && K > 0 && (pa_k_hist_dots_mapped(m, K, q, g->d_X, g->N, 0, K, src, dl, pv->buf_z, pv->ts, g->d_part, g->d_small) ||
                       pa_rt_d2h(DO, g->d_small, (size_t)K * q * sizeof(double))))
    rc = FAIL_AS(who, "%s", pa_rt_error());
  if (!rc && (pa_k_hist_dots_mapped(m, q, q, d_x, ldd, 0, q, src, dl, pv->buf_z, pv->ts, g->d_part, g->d_small) ||
              pa_rt_d2h(DN, g->d_small, (size_t)q * q * sizeof(double))))
    rc = FAIL_AS(who, "%s", pa_rt_error());
  _preAlps_ECGFree(&e);
  if (!rc) {
    const int v = pa_hist_append(&g->h, q, DO, K > 0 ? K : 1, DN, q, slots);
    if (v == PA_HIST_BAD_GRAM) rc = FAIL_AS(who, "a column of x is not finite (NaN or Inf), or x^T A x overflows");
    else if (v) rc = FAIL_AS(who, "the ring refused %d columns", q);
  }
  for (int j = 0; j < q && !rc; ++j)
    if (slots[j] >= 0 && pa_rt_d2d(g->d_X + (size_t)slots[j] * g->N, d_x + (size_t)j * ldd, (size_t)g->N * sizeof(double)))
      rc = FAIL_AS(who, "%s", pa_rt_error());
  if (pa_rt_sync() && !rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  pa_rt_free(tmp);
  if (!rc) g->appends += q;
  return rc;
}

static int project(const char* who, int nrhs, const double* b, int ldb, double* x0, int ldx0, int device, double rtol,
                   int* rank, double* captured) {
  history_t* g = &g_hist;
  if (refresh(who)) return 1;
  const int K = g->h.count, q = nrhs, N = g->N;
  double* tmp; const double* d_b; int ldd;
  double gg[PA_HIST_MAX * PA_HIST_MAX], c[PA_HIST_MAX * PA_HIST_MAX], bb[PA_HIST_MAX * PA_HIST_MAX];
  if (on_device(who, b, ldb, q, device, &tmp, &d_b, &ldd)) return 1;
  /* b^T b: a NaN or an Inf anywhere in column j shows in entry (j, j) */
  int rc = pa_k_hist_dots(N, q, q, d_b, ldd, 0, q, d_b, ldd, g->d_part, g->d_small) ||
           pa_rt_d2h(bb, g->d_small, (size_t)q * q * sizeof(double));
  if (!rc && K > 0)
    rc = pa_k_hist_dots(N, K, q, g->d_X, N, g->h.head, g->h.cap, d_b, ldd, g->d_part, g->d_small) ||
         pa_rt_d2h(gg, g->d_small, (size_t)K * q * sizeof(double));
  if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  for (int j = 0; j < q && !rc; ++j)
    if (!(bb[j + q * j] - bb[j + q * j] == 0.0)) rc = FAIL_AS(who, "right-hand side %d is not finite (NaN or Inf in b)", j);
  int rk = 0;
  if (!rc) {
    const int v = pa_hist_project(&g->h, q, gg, rtol, c, &rk, captured);
    if (v == PA_HIST_BAD_GRAM) rc = FAIL_AS(who, "the Gram matrix of the history has no positive, finite diagonal entry, or holds a NaN");
    else if (v) rc = FAIL_AS(who, "the projection of %d columns was refused", q);
  }
  if (!rc) {
    double* d_out = x0;
    double* xt = NULL;
    int ldo = ldx0;
    if (!device) { xt = (double*)pa_rt_malloc((size_t)(N > 0 ? N : 1) * q * sizeof(double)); d_out = xt; ldo = N; }
    if (!d_out) rc = FAIL_AS(who, "%d columns on the device: %s", q, pa_rt_error());
    if (!rc && K == 0)
      for (int j = 0; j < q && !rc; ++j) rc = pa_rt_memset(d_out + (size_t)j * ldo, 0, (size_t)N * sizeof(double));
    else if (!rc)
      rc = pa_rt_h2d(g->d_small + 256, c, (size_t)K * q * sizeof(double)) ||
           pa_k_hist_combine(N, K, q, g->d_X, N, g->h.head, g->h.cap, g->d_small + 256, d_out, ldo);
    for (int j = 0; xt && j < q && !rc; ++j) rc = pa_rt_d2h(x0 + (size_t)j * ldx0, xt + (size_t)j * N, (size_t)N * sizeof(double));
    if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
    pa_rt_free(xt);
  }
  if (pa_rt_sync() && !rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  pa_rt_free(tmp);
  if (!rc) { *rank = rk; g->last_rank = rk; ++g->projections; }
  return rc;
}

int preAlps_SolutionHistoryAppend(int nrhs, const double* x, int ldx, int flags) {
  if (refused(__func__, 1)) return 1;
  if (flags & ~PREALPS_SYS_DEVICE) return PA_FAIL("flags = %d: only PREALPS_SYS_DEVICE applies here", flags);
  if (array_refused(__func__, pa_operator_info(), nrhs, x, ldx, "x")) return 1;
  return append(__func__, nrhs, x, ldx, (flags & PREALPS_SYS_DEVICE) != 0);
}

int preAlps_SolutionHistoryProject(int nrhs, const double* b, int ldb, double* x0, int ldx0, int flags, double rtol,
                                   int* rank, double* captured) {
  if (refused(__func__, 1)) return 1;
  if (flags & ~PREALPS_SYS_DEVICE) return PA_FAIL("flags = %d: only PREALPS_SYS_DEVICE applies here", flags);
  if (!rank) return PA_FAIL(" wrong test 'rank != NULL'");
  const pa_operator_info_t* op = pa_operator_info();
  if (array_refused(__func__, op, nrhs, b, ldb, "b") || array_refused(__func__, op, nrhs, x0, ldx0, "x0")) return 1;
  return project(__func__, nrhs, b, ldb, x0, ldx0, (flags & PREALPS_SYS_DEVICE) != 0, rtol, rank, captured);
}

int preAlps_ECGSolveSystemHistory(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, double* x, int ldx, int flags,
                                  double rtol, double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                                  double* sys_res, double* sys_res0, int* rank, int max_hist, int* n_hist) {
  if (refused(__func__, 1)) return 1;
  if (flags & ~(PREALPS_SYS_DEVICE | PREALPS_SYS_STOP_ORIGINAL)) return PA_FAIL("flags = %d holds unknown bits", flags);
  if (!ecg) return PA_FAIL(" wrong test 'ecg != NULL'");
  const pa_operator_info_t* op = pa_operator_info();
  if (array_refused(__func__, op, nrhs, b, ldb, "b") || array_refused(__func__, op, nrhs, x, ldx, "x")) return 1;
  if (ecg->enlFac < 1 || ecg->enlFac % nrhs != 0)
    return PA_FAIL("the enlarging factor %d is not a multiple of nrhs = %d", ecg->enlFac, nrhs);
  const int device = (flags & PREALPS_SYS_DEVICE) != 0, N = op->N;
  const size_t bytes = (size_t)(N > 0 ? N : 1) * nrhs * sizeof(double);
  double* x0 = device ? (double*)pa_rt_malloc(bytes) : (double*)malloc(bytes);
  if (!x0) return PA_FAIL("%d start vectors: %s", nrhs, device ? pa_rt_error() : "out of host memory");
  int rk = 0, nh = 0;
  int rc = project(__func__, nrhs, b, ldb, x0, N, device, rtol, &rk, NULL);
  double nb[PA_HIST_MAX];
  if (!sys_normb) sys_normb = nb;
  if (!rc) rc = pa_ecg_solve_system_from(__func__, ecg, nrhs, b, ldb, rk > 0 ? x0 : NULL, N, x, ldx, flags, res_hist, bs_hist,
                                         sys_hist, sys_normb, sys_res, sys_res0, max_hist, &nh);
  /* a cold start: the start residual is the right-hand side (one system under the library's own test reports the
   * relative 1 there) */
  for (int j = 0; !rc && rk == 0 && sys_res0 && j < nrhs; ++j) sys_res0[j] = sys_normb[j];
  if (device) pa_rt_free(x0); else free(x0);
  if (rc) return 1;
  if (rank) *rank = rk;
  if (n_hist) *n_hist = nh;
  /* (a start that already met every threshold came back as x: span(Xh) holds it already) */
  return ecg->iter > 0 ? append(__func__, nrhs, x, ldx, device) : 0;
}
