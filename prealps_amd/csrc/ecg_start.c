/*
 * ecg_start.c -- the start of one or several systems on an ECG solver (with or without a guess, in the solver's
 * units or the caller's, on one or several ranks), their per-system norms, and their finish.
 *
 * ---- several right-hand sides --------------------------------------------------------------------------------
 * The block iteration started from R0 = [b_1 | ... | b_k]: nrhs = k systems, s = enlFac / k columns each, system j in
 * the columns j*s .. j*s + s - 1, a row of part p puts b_j into column j*s + (p % s).  The iteration itself is the
 * one of a single system at the same enlarging factor, launch for launch; what differs is the start (on the device:
 * pa_k_multi_start), the stopping test (every system against its own right-hand side, from the sums
 * pa_k_group_norms leaves behind each update) and the finish (pa_k_rowsum_groups).  nrhs = 1 is
 * preAlps_ECGInitialize.
 *   With an initial guess (x0 != NULL, preAlps_ECGInitializeGuess) only the start differs again: X0 goes into X by the
 * same placement rule (pa_k_guess_split), so the sum of a system's columns is x0_j bit for bit; A X0 is one plain
 * product of the library at the solver's width into the Z panel, issued before pa_ecg_reset_done so that no Gram block is
 * asked of it; pa_k_guess_start writes R0 = the split of b_j - (the sum of system j's columns of A X0) and leaves the
 * sums of b_j^2 and of R0(:, c)^2; the Z panel and the partial sums are zeroed again, so the pool is what
 * pa_ecg_reset_state leaves but for X and R.  Every later update keeps sum_c R(:, c) = b_j - A sum_c X(:, c).  who: the
 * entry point the refusals name.
 *   Several processes: every rank passes its own rows, A X0 is the distributed product, the start's local sums are
 * reduced in one all-reduce, and in the iteration the per-system sums ride on the collective of the residual norm
 * (pv->ride); what one rank alone can find wrong is agreed on before any rank returns (pa_ranks_agree).
 *   The caller's own system on several processes: b, x0 and x stay the caller's global arrays, the gather and the
 * scatter touch the rows this rank owns, the caller's-units sums of the start take one more all-reduce
 * (reduce_system_sums), and in the iteration they ride like the sums of several systems (pv->ride_sys).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ecg_priv.h"

#define FAIL_AS(who, ...) pa_fail_at(who, __VA_ARGS__)

/* The column of its system that every local row starts in: p % s for a row of part p, p the GLOBAL index of the part
 * (part0 .. part1 - 1 on this process; rowPos is global, row_off the first row owned), so that the shards of several
 * processes together hold the placement of one process.  pcol: m ints. */
static void system_columns(const pa_operator_info_t* op, int s, int* pcol) {
  for (int p = op->part0; p < op->part1; ++p) {
    int base = op->rowPos[p] - op->row_off, l = op->rowPos[p + 1] - op->rowPos[p];
    for (int i = 0; i < l; ++i) pcol[base + i] = p % s;
  }
}
int preAlps_hip_system_columns(int s, int* pcol) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built first");
  if (s < 1 || !pcol) return PA_FAIL(" wrong test 's >= 1 && pcol != NULL'");
  system_columns(op, s, pcol);
  return 0;
}
/* Collective over the process group: 1 on every process as soon as `bad` is nonzero on one (a max of one flag, as a
 * sum through the all-reduce hook; pa_mpi_agree when the library runs under its own MPI binding).  One process, and
 * the rehearsal of one shard, have nobody to ask.  The word is device memory like everything the hook is handed; in
 * plan-only mode, where there is no device, it is a host word.  word: a device word the caller already holds (the
 * solver's pool), NULL: one is allocated.  The collective is entered whatever the upload of the flag returned -- a
 * process whose copy failed reports its failure afterwards, its peers are not left waiting for it; only a process
 * that holds no word and cannot allocate one (8 bytes) has nothing to hand to the hook and fails alone. */
int pa_ranks_agree(int bad, double* word) {
  if (pa_world_size() == 1 || pa_comm_is_loopback()) return bad != 0;
  if (pa_mpi_active()) return pa_mpi_agree(bad);
  double h = bad ? 1.0 : 0.0;
  if (pa_operator_plan_only()) return pa_allreduce(&h, 1) || h != 0.0;
  double* d = word ? word : (double*)pa_rt_malloc(sizeof(double));
  if (!d) return 1;
  const int up = pa_rt_h2d(d, &h, sizeof(double));
  const int rc = pa_allreduce(d, 1) || up || pa_rt_d2h(&h, d, sizeof(double));
  if (!word) pa_rt_free(d);
  return rc || h != 0.0;
}

/* One start, as its stages see it.  multi: several processes (the one-shard rehearsal of preAlps_hip_loopback counts as
 * one of several): every rank passes its own rows.  What a rank finds wrong with ITS arguments or resources is a local
 * verdict: it does not return on it but takes it to pa_ranks_agree, so that either every rank goes on or every rank
 * returns the refusal and none is left waiting in a collective.  One process: every refusal returns at once. */
typedef struct {
  const char* who; preAlps_ECG_t* ecg; ecg_priv_t* pv; const pa_operator_info_t* op;
  int k, s, m, multi;
  const double* rhs; int ldrhs; const double* x0; int ldx0; const sys_in_t* sys;
  size_t mm, cols;        /* max(m, 1); columns of the staging array: k, with a guess 2k */
  size_t nn;              /* max(N, 1): the rows of the caller's own arrays (one process: N = m) */
  const int* d_src;       /* the caller's own system: the operator's row map */
  int gblk;               /* ... and the blocks of partial sums its gather left in d_sys_part */
} start_t;
/* The staging buffers of a start: B (and X0) go up once (m*k doubles each) with p % s of every row; the kernels write R0
 * (and X0's panel) and leave the sums of squares.  d_raw: the caller's host arrays go up as they are, then through the
 * gather (whole, the N rows of every column: on several processes the gather then picks the rows this rank owns, and the
 * ranks need no host pass over the permutation); device arrays are gathered where they lie.  gblk: the blocks of partial
 * sums the gather left in d_sys_part.  h_b1: one system in the caller's units: its scaled right-hand
 * side comes back for the host sum (m doubles, once per solve).  d_X0 / d_pcol lie in d_B's allocation. */
typedef struct { int* pcol; double* d_B; double* d_raw; double* h_b1; double* d_X0; int* d_pcol; int gblk; } staging_t;
static void staging_release(staging_t* st) {
  pa_rt_free(st->d_B);
  pa_rt_free(st->d_raw);
  free(st->pcol);
  free(st->h_b1);
  memset(st, 0, sizeof(*st));
}
static int staging_acquire(const start_t* c, staging_t* st) {   /* 1: a buffer is missing (the caller reports it) */
  const sys_in_t* sys = c->sys;
  memset(st, 0, sizeof(*st));
  st->pcol = (int*)malloc(c->mm * sizeof(int));
  st->d_B = (double*)pa_rt_malloc(c->mm * c->cols * sizeof(double) + c->mm * sizeof(int));
  st->d_raw = (sys && !sys->device) ? (double*)pa_rt_malloc(c->nn * c->cols * sizeof(double)) : NULL;
  st->h_b1 = (sys && c->k == 1) ? (double*)malloc(c->mm * sizeof(double)) : NULL;
  if (!st->pcol || !st->d_B || (sys && !sys->device && !st->d_raw) || (sys && c->k == 1 && !st->h_b1)) return 1;
  st->d_pcol = (int*)(st->d_B + c->mm * c->cols);
  st->d_X0 = c->x0 ? st->d_B + c->mm * c->k : NULL;
  return 0;
}

/* The columns and B on the device; the caller's own system: b (and x0) through the gather, which leaves the caller's
 * ||b_j||^2.  With a guess: X0 as well, and its split into the X panel. */
static int upload_and_gather(const start_t* c, staging_t* st) {
  const sys_in_t* sys = c->sys;
  ecg_priv_t* pv = c->pv;
  const int k = c->k, m = c->m;
  system_columns(c->op, c->s, st->pcol);
  int rc = pa_rt_h2d(st->d_pcol, st->pcol, (size_t)m * sizeof(int));
  if (sys) {
    const double* gb = sys->b; const double* gx = c->x0;
    int gldb = sys->ldb, gldx = c->ldx0;
    const int N = c->op->N;
    if (!sys->device) {
      for (int j = 0; j < k && !rc; ++j) rc = pa_rt_h2d(st->d_raw + (size_t)j * N, sys->b + (size_t)j * sys->ldb, (size_t)N * sizeof(double));
      for (int j = 0; c->x0 && j < k && !rc; ++j)
        rc = pa_rt_h2d(st->d_raw + (size_t)(k + j) * N, c->x0 + (size_t)j * c->ldx0, (size_t)N * sizeof(double));
      gb = st->d_raw; gx = c->x0 ? st->d_raw + c->nn * k : NULL; gldb = gldx = N;
    }
    rc = rc || pa_k_sys_gather(m, pv->ts, k, c->d_src, pv->d_dl, gb, gldb, gx, gldx, st->d_B, st->d_X0, pv->d_sys_part, &st->gblk) ||
         /* (several processes: the partial sums wait in d_sys_part for reduce_system_sums) */
         (!c->multi && pa_k_group_norms(pv->d_sys_part, st->gblk, pv->ts, k, 1, pv->d_grp + 32, pv->h_grp + 32));
  } else if (c->ldrhs == m) rc = rc || pa_rt_h2d(st->d_B, c->rhs, (size_t)m * k * sizeof(double));
  else for (int j = 0; j < k && !rc; ++j) rc = pa_rt_h2d(st->d_B + (size_t)j * m, c->rhs + (size_t)j * c->ldrhs, (size_t)m * sizeof(double));
  if (c->x0) {
    /* (the caller's system: the gather has filled d_X0) */
    if (!sys && c->ldx0 == m) rc = rc || pa_rt_h2d(st->d_X0, c->x0, (size_t)m * k * sizeof(double));
    else if (!sys) for (int j = 0; j < k && !rc; ++j) rc = pa_rt_h2d(st->d_X0 + (size_t)j * m, c->x0 + (size_t)j * c->ldx0, (size_t)m * sizeof(double));
    rc = rc || pa_k_guess_split(m, pv->ts, k, c->s, st->d_X0, m, st->d_pcol, pv->d_X);
  }
  return rc ? FAIL_AS(c->who, "%s", pa_rt_error()) : 0;
}

/* Several processes: the local sums of b_j^2 and of R0(:, c)^2 go into d_grp[1 ..) (device only), where one
 * all-reduce takes them; one process: into d_grp and its pinned mirror, as ever. */
static int start_without_guess(const start_t* c, staging_t* st) {
  ecg_priv_t* pv = c->pv;
  int nblk = 0;
  const int rc = pa_k_multi_start(c->m, pv->ts, c->k, c->s, st->d_B, c->m, st->d_pcol, pv->d_R, pv->d_rtr_part, &nblk) ||
       pa_k_group_norms(pv->d_rtr_part, nblk, pv->ts, c->k, 1, c->multi ? pv->d_grp + 1 : pv->d_grp + 16, c->multi ? NULL : pv->h_grp + 16) ||
       pa_rt_sync();
  return rc ? FAIL_AS(c->who, "%s", pa_rt_error()) : 0;
}
/* rc: what this process has met so far.  START_QUIT: the agreement ahead of the product said that a process cannot
 * go on, so every process leaves the start here, and no collective follows. */
enum { START_QUIT = 2 };
static int start_from_guess(const start_t* c, staging_t* st, int rc) {
  ecg_priv_t* pv = c->pv;
  const int k = c->k, s = c->s, m = c->m, multi = c->multi;
  double* const d_red = pv->d_grp;
  int nblk = 0;
  /* A X0 is the distributed product, with its halo exchange: no process enters it unless all of them do */
  if (multi && pa_ranks_agree(rc, d_red + 47)) {
    if (!rc) FAIL_AS(c->who, "another process of the group could not stage its rows (its own message says why)");
    return START_QUIT;
  }
  /* a plain product: nothing is armed for X -> Z, and pa_ecg_reset_done has not asked the SpMM for a block yet; on
   * the fp64 values whatever the iteration reads (preAlps_hip_set_operator_precision): R0 belongs to the matrix the
   * caller gave, which is what lets a second solve from x repair the first one's rounded operator */
  if (!rc) rc = pa_operator_apply_exact(c->ecg->X, c->ecg->Z);
  if (!rc) {
    const size_t panel = c->mm * pv->ts;
    rc = pa_k_guess_start(m, pv->ts, k, s, st->d_B, m, st->d_pcol, pv->buf_z, pv->d_R, pv->d_partials, pv->d_rtr_part, &nblk) ||
         pa_k_group_norms(pv->d_partials, nblk, pv->ts, k, 1, multi ? d_red + 1 : pv->d_grp + 16, multi ? NULL : pv->h_grp + 16) ||
         pa_k_group_norms(pv->d_rtr_part, nblk, pv->ts, k, s, multi ? d_red + 1 + k : pv->d_grp, multi ? NULL : pv->h_grp) ||
         /* the scratch as pa_ecg_reset_state left it: the first update relies on empty panels, padding included */
         pa_rt_memset(pv->buf_z, 0, panel * sizeof(double)) ||
         pa_rt_memset(pv->d_partials, 0, (size_t)nblk * pv->ts * sizeof(double)) || pa_rt_sync();
    if (rc) rc = FAIL_AS(c->who, "%s", pa_rt_error());
  }
  return rc;
}

/* one system: the sum of _preAlps_ECGReset, part by part on the host, so ecg->normb has its bits */
static double sum_one_system(const start_t* c, const double* hb) {
  const pa_operator_info_t* op = c->op;
  double nb1 = 0.0;
  for (int p = op->part0; p < op->part1; ++p) {
    int base = op->rowPos[p] - op->row_off, l = op->rowPos[p + 1] - op->rowPos[p];
    double sp = 0.0;
    for (int i = 0; i < l; ++i) { double v = hb[base + i]; sp += v * v; }
    nb1 += sp;
  }
  if (!c->multi) c->pv->h_grp[16] = nb1;
  return nb1;
}
/* ONE all-reduce of [a process failed | b_0^2 .. b_k-1^2 | with a guess: r0_0^2 .. r0_k-1^2]: behind it every
 * process holds the same words, and every verdict of start_verdicts -- a right-hand side or a start residual that is
 * zero or not finite (a NaN in one process's rows is a NaN in the sum) -- falls alike on all of them.  mine: this
 * process's own failure, which travels as the first word. */
static int reduce_start_sums(const start_t* c, int mine, double nb1) {
  ecg_priv_t* pv = c->pv;
  const int k = c->k;
  double* const d_red = pv->d_grp;
  double h[1 + 2 * 16];
  const int nred = 1 + k * (c->x0 ? 2 : 1);
  int rc = mine;
  h[0] = mine ? 1.0 : 0.0; h[1] = nb1;
  /* (the collective is entered whatever the upload returned: a process whose copy failed says so afterwards) */
  const int up = pa_rt_h2d(d_red, h, (k == 1 && !mine ? 2 : 1) * sizeof(double));
  if (pa_allreduce(d_red, nred) || up || pa_rt_d2h(h, d_red, (size_t)nred * sizeof(double)))
    rc = mine ? 1 : FAIL_AS(c->who, "%s", pa_rt_error());
  else if (h[0] != 0.0) rc = mine ? 1 : FAIL_AS(c->who, "another process of the group could not form its start (its own message says why)");
  for (int j = 0; j < k && !rc; ++j) { pv->h_grp[16 + j] = h[1 + j]; if (c->x0) pv->h_grp[j] = h[1 + k + j]; }
  return rc;
}
/* The caller's metric on several processes: ONE more all-reduce, of [a process failed | the caller's b_0^2 .. b_k-1^2 |
 * the start residuals in the caller's units, k words].  The first k sums are the fold of what the gather left in
 * d_sys_part (gblk blocks), the others pa_k_sys_norms on R0 folded the same way (the stream keeps the first fold ahead of
 * the launch that writes d_sys_part again); both go to d_grp[1 ..), which the first all-reduce has done with.  Every
 * rank enters it: the verdicts ahead of it fell alike on all of them.  The global sums land in h_grp[32 ..) and
 * h_grp[0 ..), where one process finds them. */
static int reduce_system_sums(const start_t* c) {
  ecg_priv_t* pv = c->pv;
  const int k = c->k;
  double* const d_red = pv->d_grp;
  double h[1 + 2 * 16];
  int nb = 0;
  const int mine = pa_k_group_norms(pv->d_sys_part, c->gblk, pv->ts, k, 1, d_red + 1, NULL) ||
                   pa_k_sys_norms(c->m, pv->ts, k, c->s, c->ecg->R->val, pv->d_dl, pv->d_sys_part, &nb) ||
                   pa_k_group_norms(pv->d_sys_part, nb, pv->ts, k, 1, d_red + 1 + k, NULL);
  int rc = mine ? FAIL_AS(c->who, "%s", pa_rt_error()) : 0;
  h[0] = mine ? 1.0 : 0.0;
  const int up = pa_rt_h2d(d_red, h, sizeof(double));
  if (pa_allreduce(d_red, 1 + 2 * k) || up || pa_rt_d2h(h, d_red, (size_t)(1 + 2 * k) * sizeof(double)))
    rc = mine ? 1 : FAIL_AS(c->who, "%s", pa_rt_error());
  else if (h[0] != 0.0) rc = mine ? 1 : FAIL_AS(c->who, "another process of the group could not form its norms (its own message says why)");
  for (int j = 0; j < k && !rc; ++j) { pv->h_grp[32 + j] = h[1 + j]; pv->h_grp[j] = h[1 + k + j]; }
  return rc;
}
/* The verdicts on the sums in h_grp, the per-system norms, ecg->normb; *r2: with a guess, ||R0||_F^2. */
static int start_verdicts(const start_t* c, double* r2) {
  preAlps_ECG_t* ecg = c->ecg;
  ecg_priv_t* pv = c->pv;
  const char* who = c->who;
  const int k = c->k;
  int rc = 0;
  double nb2 = 0.0;
  for (int j = 0; j < k && !rc; ++j) {
    const double b2 = pv->h_grp[16 + j];
    if (c->sys && !(b2 - b2 == 0.0)) rc = FAIL_AS(who, "right-hand side %d is not finite (NaN or Inf in b)", j);
    else if (!(b2 > 0.0)) rc = FAIL_AS(who, "right-hand side %d has norm zero: its column of R0 would be empty", j);
    pv->sys_normb[j] = sqrt(b2);
    pv->sys_res[j] = pv->sys_normb[j];
    nb2 += b2;
  }
  ecg->normb = sqrt(nb2);
  if (!rc && c->x0) {
    int nzero = 0, first_zero = -1;
    for (int j = 0; j < k && !rc; ++j) {
      const double g2 = pv->h_grp[j];
      if (!(g2 - g2 == 0.0))
        rc = FAIL_AS(who, "system %d starts with a residual that is not finite (NaN or Inf in x0 or in the right-hand side)", j);
      if (g2 == 0.0) { ++nzero; if (first_zero < 0) first_zero = j; }
      pv->sys_res[j] = sqrt(g2);
      *r2 += g2;
    }
    if (!rc && nzero > 0 && nzero < k && !(c->sys && c->sys->probe))
      rc = FAIL_AS(who, "system %d starts with a zero residual beside systems that do not: its columns of the block "
                        "would be empty and P^T A P singular (solve the others without it)", first_zero);
  }
  if (!rc && pv->metric) {
    /* the caller's metric: both sides of every test in the caller's units, the start's included */
    if (c->multi) rc = reduce_system_sums(c);
    else if (pa_ecg_queue_group_norms(ecg, pv, NULL) || pa_rt_sync()) rc = FAIL_AS(who, "%s", pa_rt_error());
    for (int j = 0; j < k && !rc; ++j) {
      pv->sys_normb[j] = sqrt(pv->h_grp[32 + j]);
      pv->sys_res[j] = sqrt(pv->h_grp[j]);
    }
  }
  return rc;
}

int pa_ecg_start_systems(const char* who, preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs,
                         const double* x0, int ldx0, int* rci_request, const sys_in_t* sys) {
  /* ---- argument verdicts ---- */
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return FAIL_AS(who, "the operator must be built before the solver");
  if (!ecg || (!rhs && !sys) || !rci_request) return FAIL_AS(who, " wrong test 'ecg != NULL && rhs != NULL && rci_request != NULL'");
  if (nrhs < 1) return FAIL_AS(who, "nrhs = %d: at least one right-hand side is needed", nrhs);
  if (ecg->enlFac < 1 || ecg->enlFac % nrhs != 0)
    return FAIL_AS(who, "the enlarging factor %d is not a multiple of nrhs = %d", ecg->enlFac, nrhs);
  const int k = nrhs, s = ecg->enlFac / nrhs, m = op->m;
  if (op->nparts < s)
    return FAIL_AS(who, "Enlarging factor per system must be lower than the number of processors"
                   " in the MPI communicator! size: %d ; enlarging factor per system: %d", op->nparts, s);
  const int multi = pa_world_size() > 1 || pa_comm_is_loopback();
  int bad = 0;
  if (!sys && ldrhs < m) bad = FAIL_AS(who, "ldrhs = %d is smaller than the %d local rows", ldrhs, m);
  else if (!sys && x0 && ldx0 < m) bad = FAIL_AS(who, "ldx0 = %d is smaller than the %d local rows", ldx0, m);
  /* the caller's own system states global rows (one process: its entry has returned these already) */
  else if (sys && sys->ldb < op->N) bad = FAIL_AS(who, "ldb = %d is smaller than the %d rows of the matrix", sys->ldb, op->N);
  else if (sys && x0 && ldx0 < op->N)
    bad = FAIL_AS(who, "%s = %d is smaller than the %d rows of the matrix", sys->probe ? "ldx" : "ldx0", ldx0, op->N);
  else if (sys && sys->ldx && sys->ldx < op->N) bad = FAIL_AS(who, "ldx = %d is smaller than the %d rows of the matrix", sys->ldx, op->N);
  if (bad && !multi) return 1;
  if (ecg->ortho_alg == ORTHODIR_FUSED)
    return FAIL_AS(who, "ORTHODIR_FUSED decides inside preAlps_ECGIterate on one sum: no per-system stopping test");
  /* a shard cut for another process group (the operator was built before preAlps_hip_set_world / preAlps_hip_loopback
   * changed it) holds other rows than the sums, and the row map of the caller's own system, would assume */
  if (multi && (op->world != pa_world_size() || op->rank != pa_world_rank() || op->loopback != pa_comm_is_loopback()))
    return FAIL_AS(who, "%s need a single process (%d processes%s) or an operator built by the process group as it is now",
                   sys ? "the caller's own system, its row map and its norms"
                       : x0 ? "an initial guess and several right-hand sides" : "several right-hand sides", pa_world_size(),
                   pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "");
  if (multi && ecg->bs_red != NO_BS_RED && (k > 1 || x0 || sys))
    return FAIL_AS(who, "block-size reduction (ADAPT_BS) with %s needs a single process (%d processes%s)",
                   sys ? "the caller's own system" : x0 ? "an initial guess" : "several right-hand sides", pa_world_size(),
                   pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "");
  /* ---- acquire and agree ---- */
  if (multi) {
    if (!bad && ecg->locPbSize != m) bad = FAIL_AS(who, "locPbSize %d differs from the operator's %d rows", ecg->locPbSize, m);
    /* (plan-only mode has no device: the verdicts on the arguments are agreed on, then the start is refused) */
    const int have = !bad && !pa_operator_plan_only() && _preAlps_ECGMalloc(ecg) == 0;
    if (!bad && !pa_operator_plan_only() && !have) bad = 1;
    if (pa_ranks_agree(bad, have ? priv_of(ecg)->d_grp + 47 : NULL)) {    /* (a word of the pool; pa_ecg_reset_state zeroes it again) */
      if (have) _preAlps_ECGFree(ecg);
      return bad ? 1 : FAIL_AS(who, "another process of the group refused this start (its own message says why)");
    }
    if (pa_operator_plan_only()) return FAIL_AS(who, "the operator was built in plan-only mode (no GPU)");
  } else if (_preAlps_ECGMalloc(ecg)) return 1;
  ecg_priv_t* pv = priv_of(ecg);
  if (k == 1 && !x0 && !sys) {
    if (_preAlps_ECGReset(ecg, (double*)rhs, rci_request)) { _preAlps_ECGFree(ecg); return 1; }
    if (!(ecg->normb > 0.0)) {
      _preAlps_ECGFree(ecg);
      return FAIL_AS(who, "right-hand side 0 has norm zero: its column of R0 would be empty");
    }
    return 0;
  }
  if (ecg->locPbSize != m) {
    _preAlps_ECGFree(ecg);
    return FAIL_AS(who, "locPbSize %d differs from the operator's %d rows", ecg->locPbSize, m);
  }
  /* from here on every process of several holds a solver, and a failure of its own (rc) travels: to pa_ranks_agree ahead
   * of the product of a guess, whose halo exchange the peers would wait in, and as the first word of the one
   * all-reduce of the start's sums */
  int rc = pa_ecg_reset_state(ecg, pv, k, x0 != NULL, sys && sys->metric) ? 1 : 0;
  if (rc && !multi) { _preAlps_ECGFree(ecg); return 1; }
  start_t c = {.who = who, .ecg = ecg, .pv = pv, .op = op, .k = k, .s = s, .m = m, .multi = multi, .rhs = rhs, .ldrhs = ldrhs,
               .x0 = x0, .ldx0 = ldx0, .sys = sys, .mm = (size_t)(m > 0 ? m : 1), .nn = (size_t)(op->N > 0 ? op->N : 1), .cols = (size_t)k * (x0 ? 2 : 1)};
  if (sys && pa_operator_system_map(&c.d_src, &pv->d_dl)) {      /* (several processes: one rank's failure, so it travels) */
    if (!multi) { _preAlps_ECGFree(ecg); return 1; }
    rc = 1;
  }
  staging_t st;
  if (staging_acquire(&c, &st) && !rc)
    rc = FAIL_AS(who, "staging %d right-hand sides: %s", k, st.pcol ? pa_rt_error() : "out of host memory");
  /* ---- upload and gather, then the start ---- */
  if (!rc) rc = upload_and_gather(&c, &st);
  if (!x0 && !rc) rc = start_without_guess(&c, &st);
  if (x0) rc = start_from_guess(&c, &st, rc);
  /* ---- sums: the host sum of one system, then the one all-reduce ---- */
  if (!rc && st.h_b1 && pa_rt_d2h(st.h_b1, st.d_B, (size_t)m * sizeof(double))) rc = FAIL_AS(who, "%s", pa_rt_error());
  const double nb1 = (!rc && k == 1) ? sum_one_system(&c, sys ? st.h_b1 : rhs) : 0.0;
  c.gblk = st.gblk;
  staging_release(&st);
  if (rc == START_QUIT) { _preAlps_ECGFree(ecg); return 1; }
  if (multi) rc = reduce_start_sums(&c, rc, nb1);
  /* ---- verdicts and the caller's metric ---- */
  double r2 = 0.0;
  if (!rc) rc = start_verdicts(&c, &r2);
  if (rc) { _preAlps_ECGFree(ecg); return 1; }
  pa_ecg_reset_done(ecg, pv, rci_request);
  if (x0) ecg->res = sqrt(r2);     /* ||R0||_F; with one system this is what preAlps_ECGSystemResiduals returns */
  return 0;
}

int preAlps_ECGInitializeMulti(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, int* rci_request) {
  return pa_ecg_start_systems(__func__, ecg, nrhs, rhs, ldrhs, NULL, 0, rci_request, NULL);
}

/* x0 == NULL: preAlps_ECGInitializeMulti, the same path. */
int preAlps_ECGInitializeGuess(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, const double* x0, int ldx0,
                               int* rci_request) {
  if (!x0) return pa_ecg_start_systems("preAlps_ECGInitializeMulti", ecg, nrhs, rhs, ldrhs, NULL, 0, rci_request, NULL);
  return pa_ecg_start_systems(__func__, ecg, nrhs, rhs, ldrhs, x0, ldx0, rci_request, NULL);
}

int preAlps_ECGSystemResiduals(preAlps_ECG_t* ecg, double* sys_res, double* sys_normb) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  if (pa_ecg_flush_x(ecg, pv)) return 1;
  if (pv->nrhs > 1 || pv->metric) {
    for (int j = 0; j < (pv->nrhs > 1 ? pv->nrhs : 1); ++j) {
      if (sys_res) sys_res[j] = pv->sys_res[j];
      if (sys_normb) sys_normb[j] = pv->sys_normb[j];
    }
  } else {
    if (sys_res) sys_res[0] = ecg->res;
    if (sys_normb) sys_normb[0] = ecg->normb;
  }
  return 0;
}

int preAlps_ECGFinalizeMulti(preAlps_ECG_t* ecg, double* sol, int ldsol) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  if (!sol) return PA_FAIL(" wrong test 'sol != NULL'");
  if (ldsol < pv->m) return PA_FAIL("ldsol = %d is smaller than the %d local rows", ldsol, pv->m);
  if (pv->nrhs <= 1) return preAlps_ECGFinalize(ecg, sol);
  if (pa_ecg_flush_x(ecg, pv)) return 1;
  /* one pass over X, k sums per row, one copy to the host */
  const int m = pv->m, k = pv->nrhs;
  const size_t need = (size_t)m * k, room = pv->lay.rtr_part - pv->lay.partials;
  double* d_sol = pv->d_partials;
  double* tmp = NULL;
  double* h_tmp = NULL;
  int rc = 0;
  if (need > room) { tmp = (double*)pa_rt_malloc(need * sizeof(double)); d_sol = tmp; }
  if (ldsol != m && need > 0) h_tmp = (double*)malloc(need * sizeof(double));
  if ((need > room && !tmp) || (ldsol != m && need > 0 && !h_tmp)) rc = PA_FAIL("buffers for %d solutions", k);
  if (!rc && (pa_k_rowsum_groups(m, pv->ts, k, pv->sgrp, pv->d_X, d_sol, m) ||
              pa_rt_d2h(h_tmp ? h_tmp : sol, d_sol, need * sizeof(double))))
    rc = PA_FAIL("%s", pa_rt_error());
  if (!rc && h_tmp)
    for (int j = 0; j < k; ++j) memcpy(sol + (size_t)j * ldsol, h_tmp + (size_t)j * m, (size_t)m * sizeof(double));
  free(h_tmp);
  pa_rt_free(tmp);
  _preAlps_ECGFree(ecg);
  return rc;
}

/* The end of a system solve: the recurrence residual norms in the caller's units (one pa_k_sys_norms on R, whichever
 * metric stopped the loop: with the caller's metric the launch and the data of the last stopping test, so the same
 * bits), the solutions scattered into the caller's order and units -- as_x0: the guess itself, copied -- and the
 * solver released.  Returns after the stream has drained.
 *   Several processes: the caller's x is the global array, and this rank writes the rows it owns and no other (the
 * scatter does on the device; a host x receives them from a copy of the scattered columns, row by row of the map).
 * The norms are global: with the caller's metric they ARE the last stopping test's (pv->sys_res: reduced then, the same
 * words on every rank), otherwise this rank's sums are reduced here, in the one collective a finish has. */
int pa_ecg_finish_system(preAlps_ECG_t* ecg, const multi_args_t* mu, int as_x0) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  const pa_operator_info_t* op = pa_operator_info();
  const sys_in_t* in = mu->sys;
  const int multi = pa_world_size() > 1 || pa_comm_is_loopback();
  const int m = pv->m, k = pv->nrhs > 1 ? pv->nrhs : 1, s = pv->sgrp, N = op ? op->N : m;
  const size_t nn = (size_t)(N > 0 ? N : 1);
  const int* d_src = NULL; const double* d_dl = NULL;
  const int* h_src = op ? op->perm + op->row_off : NULL;
  double* tmp = NULL;
  double* h_tmp = NULL;
  int nb = 0;
  int rc = pa_ecg_flush_x(ecg, pv) || !op || pa_operator_system_map(&d_src, &d_dl);
  const int reduce = multi && !pv->metric;
  if (!rc && !(multi && pv->metric) &&
      (pa_k_sys_norms(m, pv->ts, k, s, ecg->R->val, d_dl, pv->d_sys_part, &nb) ||
       pa_k_group_norms(pv->d_sys_part, nb, pv->ts, k, 1, pv->d_grp, reduce ? NULL : pv->h_grp)))
    rc = PA_FAIL("%s", pa_rt_error());
  /* (entered whatever this rank has met: its peers are in it) */
  if (reduce && (pa_allreduce(pv->d_grp, k) || pa_rt_d2h(pv->h_grp, pv->d_grp, (size_t)k * sizeof(double))) && !rc)
    rc = PA_FAIL("%s", pa_rt_error());
  if (!rc && as_x0 && multi) {
    /* the rows this rank owns of the guess, bit for bit */
    if (in->device) rc = pa_k_sys_copy_rows(m, k, d_src, in->x0, in->ldx0, mu->sys_x, mu->sys_ldx);
    else for (int j = 0; j < k; ++j) for (int i = 0; i < m; ++i)
      mu->sys_x[h_src[i] + (size_t)j * mu->sys_ldx] = in->x0[h_src[i] + (size_t)j * in->ldx0];
    if (rc) rc = PA_FAIL("%s", pa_rt_error());
  } else if (!rc && as_x0) {
    for (int j = 0; j < k && !rc; ++j) {
      if (in->device) rc = pa_rt_d2d(mu->sys_x + (size_t)j * mu->sys_ldx, in->x0 + (size_t)j * in->ldx0, (size_t)m * sizeof(double));
      else memcpy(mu->sys_x + (size_t)j * mu->sys_ldx, in->x0 + (size_t)j * in->ldx0, (size_t)m * sizeof(double));
    }
    if (rc) rc = PA_FAIL("%s", pa_rt_error());
  } else if (!rc) {
    double* d_out = mu->sys_x;
    int ld = mu->sys_ldx;
    if (!in->device) {
      tmp = (double*)pa_rt_malloc(nn * k * sizeof(double));
      if (multi) h_tmp = (double*)malloc(nn * k * sizeof(double));
      if (!tmp || (multi && !h_tmp)) rc = PA_FAIL("buffers for %d solutions: %s", k, tmp ? "out of host memory" : pa_rt_error());
      d_out = tmp; ld = N;
    }
    if (!rc && pa_k_sys_scatter(m, pv->ts, k, s, pv->d_X, d_src, d_dl, d_out, ld)) rc = PA_FAIL("%s", pa_rt_error());
    /* (d_out holds the caller's rows: row src[i] of column j at src[i] + j*N, the order of the caller's x) */
    if (tmp && multi && !rc) {
      if (pa_rt_d2h(h_tmp, tmp, nn * k * sizeof(double))) rc = PA_FAIL("%s", pa_rt_error());
      for (int j = 0; j < k && !rc; ++j) for (int i = 0; i < m; ++i)
        mu->sys_x[h_src[i] + (size_t)j * mu->sys_ldx] = h_tmp[h_src[i] + (size_t)j * N];
    }
    for (int j = 0; tmp && !multi && j < k && !rc; ++j)
      if (pa_rt_d2h(mu->sys_x + (size_t)j * mu->sys_ldx, tmp + (size_t)j * N, (size_t)N * sizeof(double)))
        rc = PA_FAIL("%s", pa_rt_error());
  }
  if (!rc && pa_rt_sync()) rc = PA_FAIL("%s", pa_rt_error());
  for (int j = 0; j < k && !rc && mu->sys_res; ++j) mu->sys_res[j] = (multi && pv->metric) ? pv->sys_res[j] : sqrt(pv->h_grp[j]);
  free(h_tmp);
  pa_rt_free(tmp);
  _preAlps_ECGFree(ecg);
  return rc;
}

/* A fresh ||b_j - A x_j|| and ||b_j|| in the caller's units: one start from the guess x at s = 1 on a temporary solver
 * of width nrhs -- the gather, the library's own product, R0 -- pa_k_sys_norms on its R0, and a free.  No
 * preconditioner is needed, and nothing of an iteration is queued.  Several processes: collective; b and x are the
 * global arrays, read at the rows this rank owns (the halo of x comes through the library's exchange), and the norms
 * are the reduced ones, the same words on every rank. */
int preAlps_OperatorSystemResiduals(int nrhs, const double* b, int ldb, const double* x, int ldx, int flags, double* res,
                                    double* normb) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built first");
  if (!b || !x) return PA_FAIL(" wrong test 'b != NULL && x != NULL'");
  if (nrhs < 1 || nrhs > 16)
    return PA_FAIL("nrhs = %d: between 1 and 16 systems at a time (what the per-system arrays of a solver hold)", nrhs);
  if (flags & ~PREALPS_SYS_DEVICE) return PA_FAIL("flags = %d: only PREALPS_SYS_DEVICE applies here", flags);
  /* (several processes: the start agrees on the leading dimensions, as it does for a solve) */
  const int multi = pa_world_size() > 1 || pa_comm_is_loopback();
  if (!multi && ldb < op->N) return PA_FAIL("ldb = %d is smaller than the %d rows of the matrix", ldb, op->N);
  if (!multi && ldx < op->N) return PA_FAIL("ldx = %d is smaller than the %d rows of the matrix", ldx, op->N);
  preAlps_ECG_t e;
  memset(&e, 0, sizeof(e));
  e.globPbSize = op->N; e.locPbSize = op->m; e.enlFac = nrhs; e.maxIter = 1; e.tol = 1e-5;
  e.ortho_alg = ORTHODIR; e.bs_red = NO_BS_RED;
  const sys_in_t in = {b, ldb, x, ldx, (flags & PREALPS_SYS_DEVICE) != 0, 1, 1, 0};
  int rci = 0;
  if (pa_ecg_start_systems(__func__, &e, nrhs, NULL, 0, x, ldx, &rci, &in)) return 1;
  ecg_priv_t* pv = priv_of(&e);
  for (int j = 0; j < nrhs; ++j) {
    if (res) res[j] = pv->sys_res[j];
    if (normb) normb[j] = pv->sys_normb[j];
  }
  _preAlps_ECGFree(&e);
  return 0;
}
