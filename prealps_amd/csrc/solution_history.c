/*
 * solution_history.c -- the solution history of the built operator (preAlps_SolutionHistory*, preAlps_ECGSolveSystemHistory):
 * the device ring Xh of the last solutions in the caller's order and units, the glue around the host unit
 * ecg_history.c (ring, Gram matrix, pivoted Cholesky) and the kernels of history.hip (dots, combine).
 *   w = A x is the library's own fp64 product, formed as preAlps_OperatorSystemResiduals forms it: a temporary solver
 * of width q at s = 1, pa_k_sys_gather for (D^-1 x)[perm], pa_k_guess_split into its X panel and
 * pa_operator_apply_exact into its Z panel; the mapped dots read that panel through the operator's row map, so
 * x_i^T (A x_j) comes out in the caller's units, where it is the same number as in the scaled, permuted system.
 *   Every entry drains the library stream before it returns, as the set-up entries do.
 *   Several processes (pa_world_size() > 1, or a preAlps_hip_loopback shard): the entries are collective.  The ring is
 * Xl, the m rows this process owns (m x cap, ld max(m, 1)); b, x and x0 stay the caller's global arrays of N rows, read
 * and written at the owned rows alone (history.hip, "owned rows").  The local sums of an entry are folded behind word 0
 * of d_red and travel in ONE all-reduce (ecg_history.h: pa_hist_red_layout), so every process holds the same G and g,
 * runs the same pivoted Cholesky and reaches the same verdicts.  What one process alone can find wrong -- a leading
 * dimension, a NULL array, an allocation -- is a local verdict: ahead of a product it goes to pa_ranks_agree, so that
 * no process waits in a halo exchange the others never enter; in a projection, which has no other collective, it is
 * word 0 of the one all-reduce, as a device failure is in every entry.  All-reduces: project 1, append 2, a refresh
 * of G 2 (the agreement and the sums).
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
  int multi, m, ld;        /* several processes: the ring holds the m owned rows; ld: N, several processes max(m, 1) */
  double* d_X;             /* ld x cap, column major */
  double* d_red;           /* several processes: the PA_HIST_RED_WORDS doubles an all-reduce carries */
  double* d_part;          /* the partial sums of a dots launch */
  double* d_small;         /* [0, 256): the K x q block of a dots launch, [256, 512): the coefficients */
  long long appends, projections, refreshes;
  int last_rank;
} history_t;
static history_t g_hist;

#define FAIL_AS(who, ...) pa_fail_at(who, __VA_ARGS__)

int preAlps_SolutionHistoryFree(void) {
  if (g_hist.live) { pa_rt_sync(); pa_rt_free(g_hist.d_X); pa_rt_free(g_hist.d_part); pa_rt_free(g_hist.d_small); pa_rt_free(g_hist.d_red); }
  memset(&g_hist, 0, sizeof(g_hist));
  return 0;
}

/* 0: key is one of the history's and *value is written (all 0 without a history) */
int pa_hist_stat(const char* key, double* value) {
  const history_t* g = &g_hist;
  if (!strcmp(key, "hist_capacity")) *value = g->live ? g->h.cap : 0;
  else if (!strcmp(key, "hist_columns")) *value = g->live ? g->h.count : 0;
  else if (!strcmp(key, "hist_bytes")) *value = g->live ? 8.0 * (double)(g->multi ? g->m : g->N) * g->h.cap : 0.0;
  else if (!strcmp(key, "hist_appends")) *value = (double)g->appends;
  else if (!strcmp(key, "hist_projections")) *value = (double)g->projections;
  else if (!strcmp(key, "hist_last_rank")) *value = g->last_rank;
  else if (!strcmp(key, "hist_gram_refreshes")) *value = (double)g->refreshes;
  else if (!strcmp(key, "hist_values_epoch")) *value = g->live ? g->epoch : 0;
  else return 1;
  return 0;
}

static int is_multi(void) { return pa_world_size() > 1 || pa_comm_is_loopback(); }

/* what every entry refuses before it looks at its arrays; need_hist: a history must exist */
static int refused(const char* who, int need_hist) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return FAIL_AS(who, "the operator must be built first");
  if (pa_operator_plan_only()) return FAIL_AS(who, "the operator was built in plan-only mode (no GPU)");
  const int multi = is_multi();
  if (pa_world_size() > 1 && !pa_comm_has_allreduce())
    return FAIL_AS(who, "%d processes but no all-reduce hook: the dots of a solution history are summed through the hooks of "
                        "preAlps_hip_set_comm, preAlps_hip_rccl_init or an MPI launcher; without them it needs a single process",
                   pa_world_size());
  /* (a shard cut for another process group holds other rows than the ring and its sums would assume) */
  if (multi && (op->world != pa_world_size() || op->rank != pa_world_rank() || op->loopback != pa_comm_is_loopback()))
    return FAIL_AS(who, "%s need a single process (%d processes%s) or an operator built by the process group as it is now",
                   "a solution history, its ring of owned rows and its sums", pa_world_size(),
                   pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "");
  if (need_hist && g_hist.live && (g_hist.build != pa_operator_build_count() || g_hist.N != op->N || g_hist.multi != multi ||
                                   (multi && g_hist.m != op->m)))
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
  const int multi = is_multi(), rows = multi ? op->m : op->N;
  const size_t nn = (size_t)(rows > 0 ? rows : 1);
  n.d_X = (double*)pa_rt_malloc(nn * capacity * sizeof(double));
  n.d_part = (double*)pa_rt_malloc((multi ? pa_k_hist_owned_part_doubles() : pa_k_hist_part_doubles()) * sizeof(double));
  n.d_small = (double*)pa_rt_malloc(512 * sizeof(double));
  n.d_red = multi ? (double*)pa_rt_malloc(PA_HIST_RED_WORDS * sizeof(double)) : NULL;
  int bad = 0;
  if (!n.d_X || !n.d_part || !n.d_small || (multi && !n.d_red))
    bad = PA_FAIL("%d columns of %d rows on the device: %s", capacity, rows, pa_rt_error());
  /* (several processes: either every process holds a ring afterwards or none has changed anything) */
  if (multi ? pa_ranks_agree(bad, n.d_red) : bad) {
    pa_rt_free(n.d_X); pa_rt_free(n.d_part); pa_rt_free(n.d_small); pa_rt_free(n.d_red);
    return bad ? 1 : PA_FAIL("another process of the group could not allocate its ring (its own message says why)");
  }
  preAlps_SolutionHistoryFree();
  pa_hist_init(&n.h, capacity);
  n.multi = multi; n.m = op->m; n.ld = (int)nn;
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

/* ---- several processes --------------------------------------------------------------------------------------------
 * bad: what this process found wrong with its own arguments or resources (its message is set): it does not return on
 * it but carries it to the entry's first collective. */
#define OTHER_REFUSED "another process of the group refused this call (its own message says why)"
#define OTHER_FAILED "another process of the group could not form its sums (its own message says why)"

/* ONE all-reduce of `words` doubles of d_red, word 0 = this process failed (mine); h receives the reduced words.  Entered
 * whatever this process has met: its peers are in it. */
static int reduce_words(const char* who, int mine, int words, double* h) {
  history_t* g = &g_hist;
  int rc = mine;
  h[0] = mine ? 1.0 : 0.0;
  const int up = pa_rt_h2d(g->d_red, h, sizeof(double));
  if (pa_allreduce(g->d_red, words) || up || pa_rt_d2h(h, g->d_red, (size_t)words * sizeof(double)))
    rc = mine ? 1 : FAIL_AS(who, "%s", pa_rt_error());
  else if (h[0] != 0.0) rc = mine ? 1 : FAIL_AS(who, OTHER_FAILED);
  return rc;
}

/* product() on several processes, for the q columns of d_x (the caller's global array, read at the owned rows) or, with
 * d_x == NULL, for the q = count columns of the ring by physical slot.  The set-up is this process's own business; the
 * product with its halo exchange is queued only after pa_ranks_agree has said that every process got that far.
 * PRODUCT_QUIT: some process did not, every process leaves and no collective follows; 1: this process failed behind
 * the agreement, which travels as word 0 of the entry's all-reduce. */
enum { PRODUCT_QUIT = 2 };
static int product_ranks(const char* who, int bad, int q, const double* d_x, int ldx, preAlps_ECG_t* e, const int** src,
                         const double** dl) {
  history_t* g = &g_hist;
  const pa_operator_info_t* op = pa_operator_info();
  const int m = op->m;
  memset(e, 0, sizeof(*e));
  const int pts = pa_operator_plan_stride();
  e->globPbSize = op->N; e->locPbSize = m; e->enlFac = (pts >= q && pts <= 16) ? pts : q; e->maxIter = 1; e->tol = 1e-5;
  e->ortho_alg = ORTHODIR; e->bs_red = NO_BS_RED;
  int rc = bad;
  ecg_priv_t* pv = NULL;
  double* st = NULL;
  const size_t mm = (size_t)(m > 0 ? m : 1);
  if (!rc) rc = _preAlps_ECGMalloc(e) ? 1 : 0;
  if (!rc) { pv = priv_of(e); rc = pa_ecg_reset_state(e, pv, q, 1, 0) || pa_operator_system_map(src, dl) ? 1 : 0; }
  if (!rc) {
    st = (double*)pa_rt_malloc(2 * mm * q * sizeof(double) + mm * sizeof(int));
    if (!st) rc = FAIL_AS(who, "staging %d columns: %s", q, pa_rt_error());
  }
  if (!rc) {
    int* d_pcol = (int*)(st + 2 * mm * q);
    int gblk = 0;
    rc = pa_rt_memset(d_pcol, 0, mm * sizeof(int)) ||
         (d_x ? pa_k_sys_gather(m, pv->ts, q, *src, *dl, d_x, ldx, d_x, ldx, st, st + mm * q, pv->d_sys_part, &gblk)
              : pa_k_hist_ring_scaled(m, q, g->d_X, g->ld, *dl, st + mm * q, m)) ||
         pa_k_guess_split(m, pv->ts, q, 1, st + mm * q, m, d_pcol, pv->d_X);
    if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  }
  if (pa_ranks_agree(rc, g->d_red)) {
    if (!rc) FAIL_AS(who, OTHER_REFUSED);
    pa_rt_sync();
    pa_rt_free(st);
    return PRODUCT_QUIT;
  }
  rc = pa_operator_apply_exact(e->X, e->Z) ? 1 : 0;
  if (pa_rt_sync() && !rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  pa_rt_free(st);
  return rc;
}

/* refresh() on several processes.  0: G is current (no collective when it already was); otherwise every process returns
 * nonzero, *bad included: behind a refresh that ran, bad is known to be 0 everywhere. */
static int refresh_ranks(const char* who, int bad) {
  history_t* g = &g_hist;
  const int now = pa_operator_values_epoch();
  if (g->epoch == now) return 0;
  if (g->h.count == 0) { g->epoch = now; return 0; }
  const int K = g->h.count;
  preAlps_ECG_t e;
  const int* src; const double* dl;
  double h[PA_HIST_RED_WORDS];
  pa_hist_red_t l;
  pa_hist_red_layout(PA_HIST_RED_REFRESH, K, K, &l);
  int rc = product_ranks(who, bad, K, NULL, 0, &e, &src, &dl);
  if (rc == PRODUCT_QUIT) { _preAlps_ECGFree(&e); return 1; }
  ecg_priv_t* pv = priv_of(&e);
  if (!rc && (pa_rt_memset(g->d_red, 0, PA_HIST_RED_WORDS * sizeof(double)) || pa_k_hist_gram_owned(g->m, K, K, g->d_X, g->ld, 0, K, NULL, 0, dl, pv->buf_z, pv->ts, g->d_part, g->d_red, l.off_a, 0)))
    rc = FAIL_AS(who, "%s", pa_rt_error());
  rc = reduce_words(who, rc, l.words, h);
  _preAlps_ECGFree(&e);
  if (rc) return 1;
  pa_hist_set_gram(&g->h, h + l.off_a, K);
  g->epoch = now;
  ++g->refreshes;
  return 0;
}

/* a caller's array on the device, whole (N rows per column: the kernels pick the owned rows) */
static int append_ranks(const char* who, int bad, int nrhs, const double* x, int ldx, int device) {
  history_t* g = &g_hist;
  if (refresh_ranks(who, bad)) return 1;
  const int K = g->h.count, q = nrhs, m = g->m;
  const size_t mm = (size_t)(m > 0 ? m : 1);
  double* tmp = NULL; const double* d_x = NULL; int ldd = 0;
  double* xs = NULL;           /* the owned rows of x in local row order, m x q */
  if (!bad && on_device(who, x, ldx, q, device, &tmp, &d_x, &ldd)) bad = 1;
  if (!bad && !(xs = (double*)pa_rt_malloc(mm * q * sizeof(double)))) bad = FAIL_AS(who, "staging %d columns: %s", q, pa_rt_error());
  preAlps_ECG_t e;
  const int* src; const double* dl;
  double h[PA_HIST_RED_WORDS];
  int slots[PA_HIST_MAX];
  pa_hist_red_t l;
  pa_hist_red_layout(PA_HIST_RED_APPEND, K, q, &l);
  int rc = product_ranks(who, bad, q, d_x, ldd, &e, &src, &dl);
  if (rc == PRODUCT_QUIT) { _preAlps_ECGFree(&e); pa_rt_free(xs); pa_rt_free(tmp); return 1; }
  ecg_priv_t* pv = priv_of(&e);
  /* (the words the entry does not fill travel as zeros) */
  if (!rc && (pa_rt_memset(g->d_red, 0, PA_HIST_RED_WORDS * sizeof(double)) ||
              pa_k_hist_gather(m, g->N, q, src, d_x, ldd, NULL, PA_HIST_MAX, xs, (int)mm) ||
              pa_k_hist_gram_owned(m, K, q, g->d_X, g->ld, 0, K > 0 ? K : 1, xs, (int)mm, dl, pv->buf_z, pv->ts, g->d_part,
                                   g->d_red, l.off_a, l.off_b)))
    rc = FAIL_AS(who, "%s", pa_rt_error());
  rc = reduce_words(who, rc, l.words, h);
  _preAlps_ECGFree(&e);
  if (!rc) {
    /* (the same words on every process: the same verdict, the same slots) */
    const int v = pa_hist_append(&g->h, q, h + l.off_a, K > 0 ? K : 1, h + l.off_b, q, slots);
    if (v == PA_HIST_BAD_GRAM) rc = FAIL_AS(who, "a column of x is not finite (NaN or Inf), or x^T A x overflows");
    else if (v) rc = FAIL_AS(who, "the ring refused %d columns", q);
  }
  if (!rc && pa_k_hist_gather(m, g->N, q, src, d_x, ldd, slots, g->h.cap, g->d_X, g->ld)) rc = FAIL_AS(who, "%s", pa_rt_error());
  if (pa_rt_sync() && !rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  pa_rt_free(xs);
  pa_rt_free(tmp);
  if (!rc) g->appends += q;
  return rc;
}

static int project_ranks(const char* who, int bad, int nrhs, const double* b, int ldb, double* x0, int ldx0, int device,
                         double rtol, int* rank, double* captured) {
  history_t* g = &g_hist;
  if (refresh_ranks(who, bad)) return 1;
  const pa_operator_info_t* op = pa_operator_info();
  const int K = g->h.count, q = nrhs, N = g->N, m = g->m;
  double* tmp = NULL; const double* d_b = NULL; int ldd = 0;
  const int* src = NULL; const double* dl = NULL;
  double h[PA_HIST_RED_WORDS], c[PA_HIST_MAX * PA_HIST_MAX];
  pa_hist_red_t l;
  pa_hist_red_layout(PA_HIST_RED_PROJECT, K, q, &l);
  /* no product, so no agreement of its own: this process's verdict is word 0 of the one all-reduce */
  int rc = bad;
  if (!rc) rc = on_device(who, b, ldb, q, device, &tmp, &d_b, &ldd) || pa_operator_system_map(&src, &dl) ? 1 : 0;
  if (!rc && (pa_rt_memset(g->d_red, 0, PA_HIST_RED_WORDS * sizeof(double)) ||
              pa_k_hist_project_owned(m, N, K, q, g->d_X, g->ld, g->h.head, g->h.cap, src, d_b, ldd, g->d_part, g->d_red, l.off_a,
                                      l.off_b)))
    rc = FAIL_AS(who, "%s", pa_rt_error());
  rc = reduce_words(who, rc, l.words, h);
  /* b^T b over all rows: a NaN or an Inf in one process's rows is one in the sum, on every process */
  for (int j = 0; j < q && !rc; ++j)
    if (!(h[l.off_a + j] - h[l.off_a + j] == 0.0)) rc = FAIL_AS(who, "right-hand side %d is not finite (NaN or Inf in b)", j);
  int rk = 0;
  if (!rc) {
    const int v = pa_hist_project(&g->h, q, h + l.off_b, rtol, c, &rk, captured);
    if (v == PA_HIST_BAD_GRAM) rc = FAIL_AS(who, "the Gram matrix of the history has no positive, finite diagonal entry, or holds a NaN");
    else if (v) rc = FAIL_AS(who, "the projection of %d columns was refused", q);
  }
  if (!rc) {
    /* the owned rows of x0 and no other; a host x0 receives them row by row of the map */
    const size_t nn = (size_t)(N > 0 ? N : 1);
    const int* h_src = op->perm + op->row_off;
    double* d_out = x0;
    double* xt = NULL;
    double* h_tmp = NULL;
    int ldo = ldx0;
    if (!device) {
      xt = (double*)pa_rt_malloc(nn * q * sizeof(double));
      h_tmp = (double*)malloc(nn * q * sizeof(double));
      if (!xt || !h_tmp) rc = FAIL_AS(who, "%d columns: %s", q, xt ? "out of host memory" : pa_rt_error());
      d_out = xt; ldo = N;
    }
    if (!rc)
      rc = (K > 0 && pa_rt_h2d(g->d_small + 256, c, (size_t)K * q * sizeof(double))) ||
           pa_k_hist_combine_owned(m, N, K, q, g->d_X, g->ld, g->h.head, g->h.cap, g->d_small + 256, src, d_out, ldo) ||
           (xt && pa_rt_d2h(h_tmp, xt, nn * q * sizeof(double)));
    if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
    for (int j = 0; xt && j < q && !rc; ++j)
      for (int i = 0; i < m; ++i) x0[h_src[i] + (size_t)j * ldx0] = h_tmp[h_src[i] + (size_t)j * N];
    free(h_tmp);
    pa_rt_free(xt);
  }
  if (pa_rt_sync() && !rc) rc = FAIL_AS(who, "%s", pa_rt_error());
  pa_rt_free(tmp);
  if (!rc) { *rank = rk; g->last_rank = rk; ++g->projections; }
  return rc;
}

/* one process: a refusal returns at once; several: a NULL array or a leading dimension is this process's own verdict
 * (*bad, for the entry's first collective), the number of columns is everybody's */
static int array_verdict(const char* who, const pa_operator_info_t* op, int nrhs, const void* a, int ld, const char* name,
                         int* bad) {
  if (!is_multi()) return array_refused(who, op, nrhs, a, ld, name);
  if (nrhs < 1 || nrhs > PA_HIST_MAX) return array_refused(who, op, nrhs, a, ld, name);
  if (!*bad && array_refused(who, op, nrhs, a, ld, name)) *bad = 1;
  return 0;
}

int preAlps_SolutionHistoryAppend(int nrhs, const double* x, int ldx, int flags) {
  if (refused(__func__, 1)) return 1;
  if (flags & ~PREALPS_SYS_DEVICE) return PA_FAIL("flags = %d: only PREALPS_SYS_DEVICE applies here", flags);
  int bad = 0;
  if (array_verdict(__func__, pa_operator_info(), nrhs, x, ldx, "x", &bad)) return 1;
  if (g_hist.multi) return append_ranks(__func__, bad, nrhs, x, ldx, (flags & PREALPS_SYS_DEVICE) != 0);
  return append(__func__, nrhs, x, ldx, (flags & PREALPS_SYS_DEVICE) != 0);
}

int preAlps_SolutionHistoryProject(int nrhs, const double* b, int ldb, double* x0, int ldx0, int flags, double rtol,
                                   int* rank, double* captured) {
  if (refused(__func__, 1)) return 1;
  if (flags & ~PREALPS_SYS_DEVICE) return PA_FAIL("flags = %d: only PREALPS_SYS_DEVICE applies here", flags);
  if (!rank) return PA_FAIL(" wrong test 'rank != NULL'");
  const pa_operator_info_t* op = pa_operator_info();
  int bad = 0;
  if (array_verdict(__func__, op, nrhs, b, ldb, "b", &bad) || array_verdict(__func__, op, nrhs, x0, ldx0, "x0", &bad)) return 1;
  if (g_hist.multi) return project_ranks(__func__, bad, nrhs, b, ldb, x0, ldx0, (flags & PREALPS_SYS_DEVICE) != 0, rtol, rank, captured);
  return project(__func__, nrhs, b, ldb, x0, ldx0, (flags & PREALPS_SYS_DEVICE) != 0, rtol, rank, captured);
}

int preAlps_ECGSolveSystemHistory(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, double* x, int ldx, int flags,
                                  double rtol, double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                                  double* sys_res, double* sys_res0, int* rank, int max_hist, int* n_hist) {
  if (refused(__func__, 1)) return 1;
  if (flags & ~(PREALPS_SYS_DEVICE | PREALPS_SYS_STOP_ORIGINAL)) return PA_FAIL("flags = %d holds unknown bits", flags);
  if (!ecg) return PA_FAIL(" wrong test 'ecg != NULL'");
  const pa_operator_info_t* op = pa_operator_info();
  const int multi = g_hist.multi;
  int bad = 0;
  if (array_verdict(__func__, op, nrhs, b, ldb, "b", &bad) || array_verdict(__func__, op, nrhs, x, ldx, "x", &bad)) return 1;
  if (ecg->enlFac < 1 || ecg->enlFac % nrhs != 0)
    return PA_FAIL("the enlarging factor %d is not a multiple of nrhs = %d", ecg->enlFac, nrhs);
  /* what the solve refuses on several processes whatever its arrays hold, before the history is asked */
  if (multi && ecg->ortho_alg == ORTHODIR_FUSED)
    return PA_FAIL("ORTHODIR_FUSED decides inside preAlps_ECGIterate on one sum: no per-system stopping test");
  if (multi && ecg->bs_red != NO_BS_RED)
    return PA_FAIL("block-size reduction (ADAPT_BS) with %s needs a single process (%d processes%s)", "the caller's own system",
                   pa_world_size(), pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "");
  const int device = (flags & PREALPS_SYS_DEVICE) != 0, N = op->N;
  const size_t bytes = (size_t)(N > 0 ? N : 1) * nrhs * sizeof(double);
  /* (several processes: the rows of x0 this process does not own are neither written nor read) */
  double* x0 = device ? (double*)pa_rt_malloc(bytes) : (double*)malloc(bytes);
  if (!x0 && !bad) bad = PA_FAIL("%d start vectors: %s", nrhs, device ? pa_rt_error() : "out of host memory");
  if (bad && !multi) return 1;
  int rk = 0, nh = 0;
  int rc = multi ? project_ranks(__func__, bad, nrhs, b, ldb, x0, N, device, rtol, &rk, NULL)
                 : project(__func__, nrhs, b, ldb, x0, N, device, rtol, &rk, NULL);
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
  if (ecg->iter <= 0) return 0;         /* (the same count on every process) */
  return multi ? append_ranks(__func__, 0, nrhs, x, ldx, device) : append(__func__, nrhs, x, ldx, device);
}
