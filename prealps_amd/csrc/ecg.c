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
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pa_host.h"
#include "smalldense.h"

#define PA_ECG_MAGIC 0x45434731u

/* 1: the driver loops of this library (preAlps_ECGSolve / preAlps_ECGAdvance) replay the launches of
 * an iteration from HIP graphs captured on the first passes (see seg_begin below); -1 = decide from
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

/* The reference brackets every BLAS / MPI call with MPI_Wtime (ecg.c:316-320 ...).  Launches
 * are asynchronous here, so the host clock only sees the enqueue; with preAlps_hip_timing(1)
 * the phase's hipEvent pair is read instead (one stream sync per phase) and the timer fields
 * of preAlps_ECG_t hold device time, which is what preAlps_ECGPrint then reports. */
#define TIC(key) do { pa_time_begin(key); t0 = pa_wtime(); } while (0)
#define TAC(key, field) \
  do { double d_ = pa_time_end(key); ecg->field += d_ >= 0.0 ? d_ : pa_wtime() - t0; } while (0)

typedef struct {
  unsigned magic;
  int ts, T, m;
  size_t pool_doubles;
  /* panel buffers (device) */
  double* buf_v[2];   /* P slot, P_prev slot */
  double* buf_av[2];  /* AP slot, AP_prev slot */
  double* buf_z;
  double* d_R; double* d_X;
  /* small blocks (device): F = [alpha T^2 | beta 2T^2 | mu T^2 | rtr T^2] */
  double* d_F; double* d_alpha; double* d_beta; double* d_mu; double* d_rtr;
  double* d_res2; double* d_q;
  double* d_partials; double* d_rtr_part;
  double* d_bj_parts; int bj_cap;       /* Gram blocks left behind by the block solve (pa_k_bj_gram_arm), 32 doubles per block */
  double* d_spmm_parts; int spmm_cap;   /* Gram blocks left behind by the SpMM (pa_k_spmm_gram_arm), 32 doubles each */
  int rtr_nblk, rtr_valid;
  int* d_info; int* d_piv;
  double* h_pin;      /* pinned: [0] res2, [1..] scratch */
  int* h_pin_i;
  int rotate;         /* NO_BS_RED: rotate pointers instead of copying */
  void* ev_res;       /* recorded after the residual norm has been copied to the host */
  int fuse;           /* NO_BS_RED: two-pass first half (PREALPS_ECG_FUSE=0 keeps the four-pass one) */
  /* Lazy normalisation (Orthodir, NO_BS_RED; PREALPS_ECG_LAZY_NORM=0 switches it off):
   * P <- P U^-1 and AP <- AP U^-1 (ecg.c:434-435 of the reference) are never written.  X and R get the same update
   * from rows normalised in registers; the block solve runs on AP_raw; the Gram blocks are formed on the raw
   * panels; and the update kernel of the second half applies U^-1 (this iteration's for P and Z, the previous
   * one's for P_prev) where the reference's panels would carry it -- the same algebra, two panel writes and
   * their 66 MB per iteration less on the headline problem.  d_uu: the two factors, uu_cur: this iteration's. */
  int lazy_norm, uu_cur;
  /* D-Odir rides the same path while every direction is live (ecg->P->info.n == enlFac); the first reduction
   * writes the normalised panels (P, AP with this iteration's factor, P_prev, AP_prev with the previous one's)
   * and ends it for the rest of the solve.  z_ready: the library's own loops queue the block solve Z = M^-1 AP
   * (AP is the raw panel, which nothing rewrites) BEFORE the host waits for alpha and decides about a reduction,
   * so the wait and the SVD are hidden behind it; the loop then skips its own apply.  ev_alpha: alpha is on the host. */
  int z_ready;
  int zz_nblk;        /* partial blocks of Z^T Z the last update kernel left in d_partials (BF-Omin), 0 = none */
  void* ev_alpha;
  double* d_uu;
  int poll;           /* the host polls the word a kernel writes behind the norm instead of waiting for an event */
  double seq, sent_seq, wait_seq;   /* last number handed out / the one travelling with the current norm / awaited */
  int lazy_stop;      /* several processes: the residual norm rides on the beta all-reduce (see below) */
  double* lazy_ptr;   /* where the first half left [res2, potrf status] for that */
  /* graphs (driver loops of this library): an iteration is two segments -- 0: the first half up to
   * the residual norm, 1: preconditioner apply + second half + product -- and the panel pointers
   * rotate with period 6 (three P slots x two AP slots), so there are 2 x 6 graphs */
  int use_graphs;
  /* solve_first: the library's own loops run an Orthodir iteration with the block solve before the update (see
   * solve_first_step; PREALPS_ECG_SOLVE_FIRST, read at reset).  sf_ready: the block solve and the finish of the
   * next iteration are queued behind its product (only inside one call of those loops, see solve_first_step). */
  int solve_first, sf_ready;
  int phase;          /* iterations since the last reset, mod 6 */
  void* graph[2][6];
  unsigned char seen[2][6];
  int bj_epoch;       /* pa_bj_apply_epoch() the graphs were captured under */
  /* Several right-hand sides (preAlps_ECGInitializeMulti): nrhs systems of sgrp = enlFac / nrhs columns each, system
   * j in the columns j*sgrp .. j*sgrp + sgrp - 1.  nrhs <= 1: one system, nothing below is used.  Every launch that
   * leaves the column sums of R^2 in d_rtr_part is followed by pa_k_group_norms (queue_group_norms), which leaves
   * g_j^2 in d_grp and in the pinned words h_grp[0..nrhs); they are complete when the scalar norm is, because that
   * reaches the host through a later launch or event of the same stream.  h_grp[16..]: the start's ||b_j||^2. */
  int nrhs, sgrp;
  double* d_grp; double* h_grp;
  /* Several systems on several processes (ride; a preAlps_hip_loopback shard of such a group too): the sums are this process's share.
   * pa_k_group_norms_ride leaves them behind the pair [norm^2, potrf status] that a collective of the iteration
   * carries anyway -- grp_dst: where it last wrote, the slot behind beta with the lazy stopping test, d_res2
   * otherwise -- so that all-reduce grows by nrhs words and the iteration gains no collective; behind it the
   * nrhs global sums are copied to h_grp ahead of the event the host waits for. */
  int ride;
  double* grp_dst;
  double sys_res[16], sys_normb[16];
  /* 1: started from an initial guess (preAlps_ECGInitializeGuess): X0 is in X and R0 = split(B - A X0).  The
   * iteration is unchanged; graphs and polling are off, and preAlps_ECGAdvance, which restarts from the right-hand
   * side alone, is refused.  _preAlps_ECGReset makes the solver a cold one again. */
  int guess;
  /* The caller's own system (preAlps_ECGSolveSystem).  metric = 1: the per-system stopping test runs on the residual in
   * the caller's units, ||b_j - A x_j|| against ||b_j||, for one system as for several: every launch that has written R
   * is followed by pa_k_sys_norms on the R panel (partial sums in d_sys_part) and pa_k_group_norms with s = 1, which
   * leaves the nrhs squares in d_grp / h_grp[0..nrhs); sys_res / sys_normb are then in that metric, ecg->res and
   * ecg->normb stay the scaled Frobenius norms.  d_dl: the scaling factor of every local row (the operator's row map,
   * NULL for every other solver).  h_grp[32..]: the caller's ||b_j||^2 from pa_k_sys_gather.  Graphs and polling are
   * off, as for several systems. */
  int metric;
  const double* d_dl;
  double* d_sys_part;
} ecg_priv_t;

static ecg_priv_t* priv_of(preAlps_ECG_t* ecg) {
  if (!ecg || !ecg->iwork) return NULL;
  int T = ecg->enlFac;
  int skip = (T + 3) & ~3; /* iwork[0..T) stays the pivot array of the reference */
  ecg_priv_t* p = (ecg_priv_t*)(ecg->iwork + skip);
  return p->magic == PA_ECG_MAGIC ? p : NULL;
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

static int pa_env_flag(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static int solve_first_switch(void) { return pa_env_flag("PREALPS_ECG_SOLVE_FIRST", 1); }

/* Where the order of solve_first_step applies (the switch on): one process, Orthodir without block-size reduction,
 * the two-pass first half with lazy normalisation and the lazy stopping test, 4 columns, the Gram blocks left behind
 * by the block solve and by the SpMM, no graphs.  Everything else keeps the order of preAlps_ECGIterate. */
static int solve_first_rule(int on, int nprocs, int ortho_alg, int bs_red, int enlFac, int fuse, int lazy_norm,
                            int lazy_stop, int bj_gram, int spmm_gram, int graphs) {
  return on && nprocs == 1 && ortho_alg == ORTHODIR && bs_red == NO_BS_RED && enlFac == 4 && fuse && lazy_norm &&
         lazy_stop && bj_gram && spmm_gram && !graphs;
}
int preAlps_hip_ecg_solve_first(int nprocs, int ortho_alg, int bs_red, int enlFac, int fuse, int lazy_norm,
                                int lazy_stop, int bj_gram, int spmm_gram, int graphs) {
  return solve_first_rule(solve_first_switch(), nprocs, ortho_alg, bs_red, enlFac, fuse, lazy_norm, lazy_stop,
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
  /* pool: same order as the reference (V, AV, Z, R, X, then the small blocks);
   * Orthomin needs no P_prev / AP_prev slots (ecg.c:55-61) */
  size_t panel = (size_t)(m > 0 ? m : 1) * ts;
  int nv = (ecg->ortho_alg == ORTHOMIN) ? 1 : 2;
  size_t small = 5 * (size_t)T * T + 2 * (size_t)T * T /* q, scratch */ + 24 /* res2: the pair + 16 sums */ + 2 * (size_t)T * T /* uu */;
  size_t parts = (size_t)pa_gram_max_blocks() * (2 * (size_t)ts * ts + ts);
  /* T = 4: the library's SpMM can form [AP | R]^T P while it computes AP (one block per workgroup) */
  pv->spmm_cap = (T == 4 && ts == 4) ? pa_operator_gram_blocks(ts) : 0;
  if (pv->spmm_cap) parts += ((size_t)pv->spmm_cap + pa_finish32_scratch_blocks()) * 32;
  /* ... and the library's block solve beta = [AP | AP_prev]^T Z while Z is still in its registers (Orthodir) */
  pv->bj_cap = (T == 4 && ts == 4 && ecg->ortho_alg == ORTHODIR && pa_env_flag("PREALPS_BJ_GRAM", 1)) ? pa_bj_gram_blocks() : 0;
  if (pv->bj_cap) parts += ((size_t)pv->bj_cap + pa_finish32_scratch_blocks()) * 32;
  parts += 48;   /* d_grp: the per-system sums of several right-hand sides (and the caller's ||b_j||^2 of a system solve) */
  parts += (size_t)pa_gram_max_blocks() * ts;   /* d_sys_part: the partial sums of pa_k_sys_gather / pa_k_sys_norms */
  pv->pool_doubles = (2 * nv + 3) * panel + small + parts;
  ecg->work = (double*)pa_rt_malloc(pv->pool_doubles * sizeof(double));
  if (!ecg->work) return PA_FAIL("device pool of %zu doubles: %s", pv->pool_doubles, pa_rt_error());
  double* w = ecg->work;
  pv->buf_v[0] = w; w += panel;
  pv->buf_v[1] = (nv == 2) ? w : NULL; if (nv == 2) w += panel;
  pv->buf_av[0] = w; w += panel;
  pv->buf_av[1] = (nv == 2) ? w : NULL; if (nv == 2) w += panel;
  pv->buf_z = w; w += panel;
  pv->d_R = w; w += panel;
  pv->d_X = w; w += panel;
  pv->d_F = w; pv->d_alpha = w; pv->d_beta = w + (size_t)T * T; pv->d_mu = w + 3 * (size_t)T * T;
  pv->d_rtr = w + 4 * (size_t)T * T; w += 5 * (size_t)T * T;
  pv->d_q = w; w += 2 * (size_t)T * T;
  pv->d_res2 = w; w += 24;
  pv->d_uu = w; w += 2 * (size_t)T * T;
  pv->d_partials = w; w += (size_t)pa_gram_max_blocks() * 2 * ts * ts;
  pv->d_rtr_part = w; w += (size_t)pa_gram_max_blocks() * ts;
  pv->d_spmm_parts = pv->spmm_cap ? w : NULL;
  if (pv->spmm_cap) w += ((size_t)pv->spmm_cap + pa_finish32_scratch_blocks()) * 32;
  pv->d_bj_parts = pv->bj_cap ? w : NULL;
  if (pv->bj_cap) w += ((size_t)pv->bj_cap + pa_finish32_scratch_blocks()) * 32;
  pv->d_grp = w; w += 48;
  pv->d_sys_part = w;
  pv->d_info = (int*)pa_rt_malloc((8 + T) * sizeof(int));
  if (!pv->d_info) return PA_FAIL("device allocation failed: %s", pa_rt_error());
  pv->d_piv = pv->d_info + 8;
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
static void request_gram_from_spmm(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
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
static int reset_state(preAlps_ECG_t* ecg, ecg_priv_t* pv, int nrhs, int guess, int metric) {
  pv->nrhs = nrhs; pv->sgrp = ecg->enlFac / nrhs; pv->guess = guess; pv->metric = metric; pv->d_dl = NULL;
  /* (a loopback shard of a group of ONE is a single process in every branch of the iteration -- pa_world_size() is
   * what they read -- and has nothing to reduce: it keeps pa_k_group_norms and the pinned mirror) */
  pv->ride = nrhs > 1 && !metric && pa_world_size() > 1;
  pv->grp_dst = NULL;
  ecg->tot_t = ecg->comm_t = ecg->trsm_t = ecg->gemm_t = ecg->potrf_t = ecg->pstrf_t = 0.0;
  ecg->lapmt_t = ecg->gesvd_t = ecg->geqrf_t = ecg->ormqr_t = ecg->copy_t = 0.0;
  int M = ecg->globPbSize, m = ecg->locPbSize, t = ecg->enlFac, ts = pv->ts;
  /* pointer order back to the initial one */
  {
    size_t panel = (size_t)(m > 0 ? m : 1) * ts;
    double* w = ecg->work;
    int nv = (ecg->ortho_alg == ORTHOMIN) ? 1 : 2;
    pv->buf_v[0] = w; w += panel; if (nv == 2) { pv->buf_v[1] = w; w += panel; }
    pv->buf_av[0] = w; w += panel; if (nv == 2) { pv->buf_av[1] = w; w += panel; }
    pv->buf_z = w;
  }
  publish_pointers(ecg, pv);
  pv->rotate = (ecg->bs_red == NO_BS_RED);
  { const char* f = getenv("PREALPS_ECG_FUSE"); pv->fuse = f ? atoi(f) : 1; }
  pv->lazy_norm = pv->fuse && ecg->ortho_alg == ORTHODIR && pa_env_flag("PREALPS_ECG_LAZY_NORM", 1);
  pv->uu_cur = 0;
  pv->z_ready = 0;
  pv->solve_first = solve_first_switch();
  pv->sf_ready = 0;
  /* With more than one process every collective costs tens of microseconds.  The norm of the
   * new residual is only needed for the stopping decision, so the driver loops of this library
   * (preAlps_ECGSolve / ECGAdvance) let it travel with the beta all-reduce of the same
   * iteration and decide one half-step later; the last half-step is then simply unused.  The
   * RCI entry preAlps_ECGStoppingCriterion keeps working (it reduces the norm by itself).
   * One process: the same order saves the launch that sums the norm (it is summed with beta):
   * 2-3 us per iteration (in-process A/B), so it is the default there too; PREALPS_ECG_LAZY_STOP=0
   * decides right after the update, as the reference does. */
  { const char* f = getenv("PREALPS_ECG_LAZY_STOP");
    pv->lazy_stop = pv->fuse && ecg->bs_red == NO_BS_RED && ecg->ortho_alg != ORTHODIR_FUSED && ecg->enlFac >= 2 &&
                    (f ? atoi(f) : 1);
    pv->lazy_ptr = NULL; }
  /* graphs (opt-in: preAlps_hip_graphs(1) or PREALPS_ECG_GRAPH=1): one process, or the one-shard
   * rehearsal of preAlps_hip_loopback, whose sums are free, so the stopping test need not ride on one;
   * =2 forces them for any process group (the hooks must then be capturable: RCCL is, host-staged ones
   * are not).  Off by default because they measure SLOWER on this stack: 436.5 us per iteration against
   * 423.2 us with plain launches on the headline problem (same box, 200 iterations each; ROCm 7.2 puts
   * more idle time between the nodes of a graph than between launches queued on a stream) */
  {
    const char* ge = getenv("PREALPS_ECG_GRAPH");
    int want = g_graphs >= 0 ? g_graphs : (ge ? atoi(ge) : 0);
    if (nrhs > 1) want = 0;      /* (several systems: the group launch is not part of the captured segments) */
    if (guess) want = 0;         /* (a start from a guess: as for several systems, whatever nrhs) */
    if (metric) want = 0;        /* (the caller's metric: its two launches are not part of the segments either) */
    int group_ok = pa_world_size() == 1 || pa_comm_is_loopback() || want == 2;
    pv->use_graphs = want && group_ok && pv->rotate && pv->fuse && ecg->ortho_alg != ORTHODIR_FUSED &&
                     !pa_timing_enabled();
    if (pv->use_graphs) pv->lazy_stop = 0;
    pv->phase = 0;
  }
  /* the residual norm reaches the host through two pinned words a kernel writes; a third word behind
   * them (a sequence number) lets the host poll for them instead of waiting for an event recorded in the
   * stream.  Default with several processes, where it measures 5 us per iteration faster (one-shard
   * rehearsal: 112.5 against 117.8 us); one process: no difference (the 6 us bubble the event leaves
   * behind k_trace_finish reappears behind the block solve), so the event stays.  PREALPS_ECG_POLL=0 / 1
   * forces; graphs replay fixed arguments and keep the event. */
  { const char* f = getenv("PREALPS_ECG_POLL"); pv->poll = (f ? atoi(f) : pa_world_size() > 1) && !pv->use_graphs;
    /* several systems: the per-system sums may be queued behind the launch that writes the polled word, so the
     * host waits for the event behind both */
    if (nrhs > 1 || guess || metric) pv->poll = 0; }
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
  PA_CHECK(pa_rt_memset(ecg->work, 0, pv->pool_doubles * sizeof(double)));
  if (pv->lazy_norm) {        /* (the first update meets an empty P_prev: any factor will do, the identity is one) */
    double eye[2 * 16 * 16];
    memset(eye, 0, sizeof(eye));
    for (int k = 0; k < 2; ++k) for (int i = 0; i < t; ++i) eye[(size_t)k * t * t + i + (size_t)t * i] = 1.0;
    PA_CHECK(pa_rt_h2d(pv->d_uu, eye, 2 * (size_t)t * t * sizeof(double)));
  }
  return 0;
}
static void reset_done(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* rci_request) {
  ecg->res = 1.0; ecg->iter = 0; ecg->bs = ecg->enlFac; ecg->kbs = ecg->V->info.n;
  pv->rtr_valid = 0;
  *rci_request = 0;
  request_gram_from_spmm(ecg, pv);
}

int _preAlps_ECGReset(preAlps_ECG_t* ecg, double* rhs, int* rci_request) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver memory not allocated (_preAlps_ECGMalloc)");
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built before the solver");
  if (ecg->locPbSize != op->m) return PA_FAIL("locPbSize %d differs from the operator's %d rows", ecg->locPbSize, op->m);
  if (pv->nrhs > 1) return PA_FAIL("the solver holds %d systems: restart it with preAlps_ECGInitializeMulti", pv->nrhs);
  if (reset_state(ecg, pv, 1, 0, 0)) return 1;
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
  reset_done(ecg, pv, rci_request);
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

/* ---- several right-hand sides --------------------------------------------------------------------------------
 * The block iteration started from R0 = [b_1 | ... | b_k]: nrhs = k systems, s = enlFac / k columns each, system j in
 * the columns j*s .. j*s + s - 1, a row of part p puts b_j into column j*s + (p % s).  The iteration itself is the
 * one of a single system at the same enlarging factor, launch for launch; what differs is the start (on the device:
 * pa_k_multi_start), the stopping test (every system against its own right-hand side, from the sums
 * pa_k_group_norms leaves behind each update) and the finish (pa_k_rowsum_groups).  nrhs = 1 is
 * preAlps_ECGInitialize.
 *   With an initial guess (x0 != NULL, preAlps_ECGInitializeGuess) only the start differs again: X0 goes into X by the
 * same placement rule (pa_k_guess_split), so the sum of a system's columns is x0_j bit for bit; A X0 is one plain
 * product of the library at the solver's width into the Z panel, issued before reset_done so that no Gram block is
 * asked of it; pa_k_guess_start writes R0 = the split of b_j - (the sum of system j's columns of A X0) and leaves the
 * sums of b_j^2 and of R0(:, c)^2; the Z panel and the partial sums are zeroed again, so the pool is what reset_state
 * leaves but for X and R.  Every later update keeps sum_c R(:, c) = b_j - A sum_c X(:, c).  who: the entry point the
 * refusals name.
 *   Several processes: every rank passes its own rows, A X0 is the distributed product, the start's local sums are
 * reduced in one all-reduce, and in the iteration the per-system sums ride on the collective of the residual norm
 * (pv->ride); what one rank alone can find wrong is agreed on before any rank returns (ranks_agree). */
#define FAIL_AS(who, ...) pa_fail_at(who, __VA_ARGS__)
static int queue_group_norms(preAlps_ECG_t* ecg, ecg_priv_t* pv, double* dst);
/* The caller's own system (preAlps_ECGSolveSystem, preAlps_OperatorSystemResiduals): b and x0 hold the rows in the order
 * and units of the matrix the operator was built from, on the host or (device) on the device.  pa_k_sys_gather fills
 * the staging arrays d_B / d_X0 that the host path uploads into -- b' = dl * b[src], x0' = x0[src] / dl -- and leaves
 * the caller's ||b_j||^2; what follows the uploads is the same code.  metric: the stopping test is the caller's;
 * probe: only the start's norms are wanted, so a system that starts at exactly zero is no refusal. */
typedef struct { const double* b; int ldb; const double* x0; int ldx0; int device, metric, probe; } sys_in_t;
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
static int ranks_agree(int bad, double* word) {
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
static int start_systems(const char* who, preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs,
                         const double* x0, int ldx0, int* rci_request, const sys_in_t* sys) {
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
  /* Several processes (multi; the one-shard rehearsal of preAlps_hip_loopback counts as one of several): every rank
   * passes its own rows.  What a rank finds wrong with ITS arguments or resources is a local verdict (bad): it does
   * not return on it but takes it to ranks_agree, so that either every rank goes on or every rank returns the refusal
   * and none is left waiting in a collective.  One process: every refusal returns at once, as it always did. */
  const int multi = pa_world_size() > 1 || pa_comm_is_loopback();
  int bad = 0;
  if (!sys && ldrhs < m) bad = FAIL_AS(who, "ldrhs = %d is smaller than the %d local rows", ldrhs, m);
  else if (!sys && x0 && ldx0 < m) bad = FAIL_AS(who, "ldx0 = %d is smaller than the %d local rows", ldx0, m);
  if (bad && !multi) return 1;
  if (ecg->ortho_alg == ORTHODIR_FUSED)
    return FAIL_AS(who, "ORTHODIR_FUSED decides inside preAlps_ECGIterate on one sum: no per-system stopping test");
  /* the caller's own system states global rows; and a shard cut for another process group (the operator was built
   * before preAlps_hip_set_world / preAlps_hip_loopback changed it) holds other rows than the sums would assume */
  if (multi && (sys || op->world != pa_world_size() || op->rank != pa_world_rank() || op->loopback != pa_comm_is_loopback()))
    return FAIL_AS(who, "%s need a single process (%d processes%s)%s",
                   sys ? "the caller's own system, its row map and its norms"
                       : x0 ? "an initial guess and several right-hand sides" : "several right-hand sides", pa_world_size(),
                   pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "",
                   sys ? "" : " or an operator built by the process group as it is now");
  if (multi && ecg->bs_red != NO_BS_RED && (k > 1 || x0))
    return FAIL_AS(who, "block-size reduction (ADAPT_BS) with %s needs a single process (%d processes%s)",
                   x0 ? "an initial guess" : "several right-hand sides", pa_world_size(),
                   pa_comm_is_loopback() ? ", preAlps_hip_loopback shard" : "");
  if (multi) {
    if (!bad && ecg->locPbSize != m) bad = FAIL_AS(who, "locPbSize %d differs from the operator's %d rows", ecg->locPbSize, m);
    /* (plan-only mode has no device: the verdicts on the arguments are agreed on, then the start is refused) */
    const int have = !bad && !pa_operator_plan_only() && _preAlps_ECGMalloc(ecg) == 0;
    if (!bad && !pa_operator_plan_only() && !have) bad = 1;
    if (ranks_agree(bad, have ? priv_of(ecg)->d_grp + 47 : NULL)) {    /* (a word of the pool; reset_state zeroes it again) */
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
  /* from here on every process of several holds a solver, and a failure of its own (rc) travels: to ranks_agree ahead
   * of the product of a guess, whose halo exchange the peers would wait in, and as the first word of the one
   * all-reduce of the start's sums */
  int rc = reset_state(ecg, pv, k, x0 != NULL, sys && sys->metric) ? 1 : 0, nblk = 0;
  if (rc && !multi) { _preAlps_ECGFree(ecg); return 1; }
  const int* d_src = NULL;
  if (sys) {
    if (pa_operator_system_map(&d_src, &pv->d_dl)) { _preAlps_ECGFree(ecg); return 1; }
  }
  /* B (and X0) go up once (m*k doubles each) with p % s of every row; the kernels write R0 (and X0's panel) and leave
   * the sums of squares */
  const size_t mm = (size_t)(m > 0 ? m : 1), cols = (size_t)k * (x0 ? 2 : 1);
  int* pcol = (int*)malloc(mm * sizeof(int));
  double* d_B = (double*)pa_rt_malloc(mm * cols * sizeof(double) + mm * sizeof(int));
  /* the caller's host arrays go up as they are, then through the gather; device arrays are gathered where they lie */
  double* d_raw = (sys && !sys->device) ? (double*)pa_rt_malloc(mm * cols * sizeof(double)) : NULL;
  double* h_b1 = (sys && k == 1) ? (double*)malloc(mm * sizeof(double)) : NULL;    /* (see the sum of one system below) */
  /* several processes: the local sums of b_j^2 and of R0(:, c)^2 go into d_red[1 ..) (device only), where one
   * all-reduce takes them; one process: into d_grp and its pinned mirror, as ever */
  double* const d_red = pv->d_grp;
  if (!rc && (!pcol || !d_B || (sys && !sys->device && !d_raw) || (sys && k == 1 && !h_b1)))
    rc = FAIL_AS(who, "staging %d right-hand sides: %s", k, pcol ? pa_rt_error() : "out of host memory");
  if (!rc) {
    int* d_pcol = (int*)(d_B + mm * cols);
    double* d_X0 = x0 ? d_B + mm * k : NULL;
    system_columns(op, s, pcol);
    rc = pa_rt_h2d(d_pcol, pcol, (size_t)m * sizeof(int));
    if (sys) {
      const double* gb = sys->b; const double* gx = x0;
      int gldb = sys->ldb, gldx = ldx0, gblk = 0;
      if (!sys->device) {
        for (int j = 0; j < k && !rc; ++j) rc = pa_rt_h2d(d_raw + (size_t)j * m, sys->b + (size_t)j * sys->ldb, (size_t)m * sizeof(double));
        for (int j = 0; x0 && j < k && !rc; ++j)
          rc = pa_rt_h2d(d_raw + (size_t)(k + j) * m, x0 + (size_t)j * ldx0, (size_t)m * sizeof(double));
        gb = d_raw; gx = x0 ? d_raw + mm * k : NULL; gldb = gldx = m;
      }
      rc = rc || pa_k_sys_gather(m, pv->ts, k, d_src, pv->d_dl, gb, gldb, gx, gldx, d_B, d_X0, pv->d_sys_part, &gblk) ||
           pa_k_group_norms(pv->d_sys_part, gblk, pv->ts, k, 1, pv->d_grp + 32, pv->h_grp + 32);
    } else if (ldrhs == m) rc = rc || pa_rt_h2d(d_B, rhs, (size_t)m * k * sizeof(double));
    else for (int j = 0; j < k && !rc; ++j) rc = pa_rt_h2d(d_B + (size_t)j * m, rhs + (size_t)j * ldrhs, (size_t)m * sizeof(double));
    if (!x0) {
      rc = rc || pa_k_multi_start(m, pv->ts, k, s, d_B, m, d_pcol, pv->d_R, pv->d_rtr_part, &nblk) ||
           pa_k_group_norms(pv->d_rtr_part, nblk, pv->ts, k, 1, multi ? d_red + 1 : pv->d_grp + 16, multi ? NULL : pv->h_grp + 16) ||
           pa_rt_sync();
      if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
    } else {
      /* (the caller's system: the gather has filled d_X0) */
      if (!sys && ldx0 == m) rc = rc || pa_rt_h2d(d_X0, x0, (size_t)m * k * sizeof(double));
      else if (!sys) for (int j = 0; j < k && !rc; ++j) rc = pa_rt_h2d(d_X0 + (size_t)j * m, x0 + (size_t)j * ldx0, (size_t)m * sizeof(double));
      rc = rc || pa_k_guess_split(m, pv->ts, k, s, d_X0, m, d_pcol, pv->d_X);
      if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
    }
  }
  if (x0) {
    /* A X0 is the distributed product, with its halo exchange: no process enters it unless all of them do */
    if (multi && ranks_agree(rc, d_red + 47)) {
      if (!rc) FAIL_AS(who, "another process of the group could not stage its rows (its own message says why)");
      pa_rt_free(d_B); pa_rt_free(d_raw); free(pcol); free(h_b1);
      _preAlps_ECGFree(ecg);
      return 1;
    }
    /* a plain product: nothing is armed for X -> Z, and reset_done has not asked the SpMM for a block yet */
    if (!rc) rc = preAlps_BlockOperator(ecg->X, ecg->Z);
    if (!rc) {
      const size_t panel = mm * pv->ts;
      const int* d_pcol = (const int*)(d_B + mm * cols);
      rc = pa_k_guess_start(m, pv->ts, k, s, d_B, m, d_pcol, pv->buf_z, pv->d_R, pv->d_partials, pv->d_rtr_part, &nblk) ||
           pa_k_group_norms(pv->d_partials, nblk, pv->ts, k, 1, multi ? d_red + 1 : pv->d_grp + 16, multi ? NULL : pv->h_grp + 16) ||
           pa_k_group_norms(pv->d_rtr_part, nblk, pv->ts, k, s, multi ? d_red + 1 + k : pv->d_grp, multi ? NULL : pv->h_grp) ||
           /* the scratch as reset_state left it: the first update relies on empty panels, padding included */
           pa_rt_memset(pv->buf_z, 0, panel * sizeof(double)) ||
           pa_rt_memset(pv->d_partials, 0, (size_t)nblk * pv->ts * sizeof(double)) || pa_rt_sync();
      if (rc) rc = FAIL_AS(who, "%s", pa_rt_error());
    }
  }
  /* one system: its scaled right-hand side comes back for the host sum below (m doubles, once per solve) */
  if (!rc && h_b1 && pa_rt_d2h(h_b1, d_B, (size_t)m * sizeof(double))) rc = FAIL_AS(who, "%s", pa_rt_error());
  pa_rt_free(d_B);
  pa_rt_free(d_raw);
  free(pcol);
  double r2 = 0.0, nb1 = 0.0;
  if (!rc && k == 1) {   /* one system: the sum of _preAlps_ECGReset, part by part on the host, so ecg->normb has its bits */
    const double* hb = sys ? h_b1 : rhs;
    for (int p = op->part0; p < op->part1; ++p) {
      int base = op->rowPos[p] - op->row_off, l = op->rowPos[p + 1] - op->rowPos[p];
      double sp = 0.0;
      for (int i = 0; i < l; ++i) { double v = hb[base + i]; sp += v * v; }
      nb1 += sp;
    }
    if (!multi) pv->h_grp[16] = nb1;
  }
  if (multi) {
    /* ONE all-reduce of [a process failed | b_0^2 .. b_k-1^2 | with a guess: r0_0^2 .. r0_k-1^2]: behind it every
     * process holds the same words, and every verdict below -- a right-hand side or a start residual that is zero or
     * not finite (a NaN in one process's rows is a NaN in the sum) -- falls alike on all of them */
    double h[1 + 2 * 16];
    const int nred = 1 + k * (x0 ? 2 : 1), mine = rc;
    h[0] = mine ? 1.0 : 0.0; h[1] = nb1;
    /* (the collective is entered whatever the upload returned: a process whose copy failed says so afterwards) */
    const int up = pa_rt_h2d(d_red, h, (k == 1 && !mine ? 2 : 1) * sizeof(double));
    if (pa_allreduce(d_red, nred) || up || pa_rt_d2h(h, d_red, (size_t)nred * sizeof(double)))
      rc = mine ? 1 : FAIL_AS(who, "%s", pa_rt_error());
    else if (h[0] != 0.0) rc = mine ? 1 : FAIL_AS(who, "another process of the group could not form its start (its own message says why)");
    for (int j = 0; j < k && !rc; ++j) { pv->h_grp[16 + j] = h[1 + j]; if (x0) pv->h_grp[j] = h[1 + k + j]; }
  }
  if (!rc) {
    double nb2 = 0.0;
    for (int j = 0; j < k && !rc; ++j) {
      const double b2 = pv->h_grp[16 + j];
      if (sys && !(b2 - b2 == 0.0)) rc = FAIL_AS(who, "right-hand side %d is not finite (NaN or Inf in b)", j);
      else if (!(b2 > 0.0)) rc = FAIL_AS(who, "right-hand side %d has norm zero: its column of R0 would be empty", j);
      pv->sys_normb[j] = sqrt(b2);
      pv->sys_res[j] = pv->sys_normb[j];
      nb2 += b2;
    }
    ecg->normb = sqrt(nb2);
  }
  free(h_b1);
  if (!rc && x0) {
    int nzero = 0, first_zero = -1;
    for (int j = 0; j < k && !rc; ++j) {
      const double g2 = pv->h_grp[j];
      if (!(g2 - g2 == 0.0))
        rc = FAIL_AS(who, "system %d starts with a residual that is not finite (NaN or Inf in x0 or in the right-hand side)", j);
      if (g2 == 0.0) { ++nzero; if (first_zero < 0) first_zero = j; }
      pv->sys_res[j] = sqrt(g2);
      r2 += g2;
    }
    if (!rc && nzero > 0 && nzero < k && !(sys && sys->probe))
      rc = FAIL_AS(who, "system %d starts with a zero residual beside systems that do not: its columns of the block "
                        "would be empty and P^T A P singular (solve the others without it)", first_zero);
  }
  if (!rc && pv->metric) {
    /* the caller's metric: both sides of every test in the caller's units, the start's included */
    if (queue_group_norms(ecg, pv, NULL) || pa_rt_sync()) rc = FAIL_AS(who, "%s", pa_rt_error());
    for (int j = 0; j < k && !rc; ++j) {
      pv->sys_normb[j] = sqrt(pv->h_grp[32 + j]);
      pv->sys_res[j] = sqrt(pv->h_grp[j]);
    }
  }
  if (rc) { _preAlps_ECGFree(ecg); return 1; }
  reset_done(ecg, pv, rci_request);
  if (x0) ecg->res = sqrt(r2);     /* ||R0||_F; with one system this is what preAlps_ECGSystemResiduals returns */
  return 0;
}

int preAlps_ECGInitializeMulti(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, int* rci_request) {
  return start_systems(__func__, ecg, nrhs, rhs, ldrhs, NULL, 0, rci_request, NULL);
}

/* x0 == NULL: preAlps_ECGInitializeMulti, the same path. */
int preAlps_ECGInitializeGuess(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, const double* x0, int ldx0,
                               int* rci_request) {
  if (!x0) return start_systems("preAlps_ECGInitializeMulti", ecg, nrhs, rhs, ldrhs, NULL, 0, rci_request, NULL);
  return start_systems(__func__, ecg, nrhs, rhs, ldrhs, x0, ldx0, rci_request, NULL);
}

int preAlps_ECGSystemResiduals(preAlps_ECG_t* ecg, double* sys_res, double* sys_normb) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
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
  /* one pass over X, k sums per row, one copy to the host */
  const int m = pv->m, k = pv->nrhs;
  const size_t need = (size_t)m * k, room = (size_t)pa_gram_max_blocks() * 2 * pv->ts * pv->ts;
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
static int stopping_end(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* stop);
/* Several systems: the per-system sums, right behind the launch that left the column sums in d_rtr_part (rtr_nblk
 * blocks) and so ahead of whatever carries the scalar norm to the host. */
/* The caller's metric: the R panel itself is read instead -- every call site comes behind the launch that wrote this
 * iteration's R, on the same stream (the update kernels of fused_update, update_iterate and solve_first_step; in
 * stopping_queue nothing has touched R since); R never takes part in the rotation of the direction panels, and its
 * pointer is taken from the descriptor at the moment of the launch. */
/* Several processes (pv->ride): the sums are local, and go behind the pair [norm^2, status] at `dst` that the next
 * collective carries (d_res2, or the slot behind beta when the norm is summed with beta); dst is unused otherwise. */
static int queue_group_norms(preAlps_ECG_t* ecg, ecg_priv_t* pv, double* dst) {
  if (pv->ride) {
    PA_CHECK(pa_k_group_norms_ride(pv->d_rtr_part, pv->rtr_nblk, pv->ts, pv->nrhs, pv->sgrp, pv->d_info, dst));
    pv->grp_dst = dst;
  } else if (pv->metric) {
    int nb = 0;
    const int k = pv->nrhs > 1 ? pv->nrhs : 1;
    PA_CHECK(pa_k_sys_norms(pv->m, pv->ts, k, pv->sgrp, ecg->R->val, pv->d_dl, pv->d_sys_part, &nb));
    PA_CHECK(pa_k_group_norms(pv->d_sys_part, nb, pv->ts, k, 1, pv->d_grp, pv->h_grp));
  } else if (pv->nrhs > 1)
    PA_CHECK(pa_k_group_norms(pv->d_rtr_part, pv->rtr_nblk, pv->ts, pv->nrhs, pv->sgrp, pv->d_grp, pv->h_grp));
  return 0;
}
static int stopping_queue(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  int T = ecg->enlFac;
  int single = pa_world_size() == 1;
  if (pv->ride) {
    /* several systems on several processes: pa_k_group_norms_ride has left [norm^2, status | g_0^2 .. g_k-1^2] of
     * this process at grp_dst behind the last update (from R itself when nothing is left of one); ONE all-reduce
     * of 2 + k words where one system reduces its norm, and the k global sums follow the pair to the host */
    if (!pv->rtr_valid) {
      PA_CHECK(pa_k_colnorm2(pv->m, pv->ts, pv->d_R, pv->d_rtr_part, &pv->rtr_nblk));
      if (queue_group_norms(ecg, pv, pv->d_res2)) return 1;
    }
    double* src = pv->grp_dst;
    double t0;
    TIC(PA_T_COMM);
    if (pa_allreduce(src, 2 + pv->nrhs)) return 1;
    TAC(PA_T_COMM, comm_t);
    PA_CHECK(pa_rt_d2h_async(pv->h_pin, src, 2 * sizeof(double)));
    PA_CHECK(pa_rt_d2h_async(pv->h_grp, src + 2, (size_t)pv->nrhs * sizeof(double)));
    pv->wait_seq = pv->sent_seq = 0.0;
    pv->rtr_valid = 0;
    return 0;
  }
  if (pv->rtr_valid < 2) {
    if (!pv->rtr_valid) {
      PA_CHECK(pa_k_colnorm2(pv->m, pv->ts, pv->d_R, pv->d_rtr_part, &pv->rtr_nblk));
      if (queue_group_norms(ecg, pv, NULL)) return 1;
    }
    if (single && pv->rtr_valid == 1) {
      /* column sums left by the update kernel (lazy stopping test), one process: the sum goes straight to
       * the pinned words, as it does from the update kernel's own launch without the lazy test */
      pv->sent_seq = 0.0;
      if (pv->poll) { pv->sent_seq = (pv->seq += 1.0); pa_k_note_seq(pv->sent_seq); }
      PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->d_res2, pv->d_info, pv->h_pin));
      pv->rtr_valid = 2;
    } else {
      PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->d_res2, pv->d_info, NULL));
      pv->rtr_valid = 3;   /* summed, but not on the host yet */
    }
  }
  /* rtr_valid == 2: the update kernel summed the norm itself and, in a single-process run,
   * already wrote it to the pinned words the host reads */
  pv->wait_seq = 0.0;
  if (!single || pv->rtr_valid == 3) {
    double* src = (pv->rtr_valid == 2 && pv->lazy_ptr) ? pv->lazy_ptr : pv->d_res2;
    double t0;
    TIC(PA_T_COMM);
    if (pa_allreduce(src, 1)) return 1;
    TAC(PA_T_COMM, comm_t);
    PA_CHECK(pa_rt_d2h_async(pv->h_pin, src, 2 * sizeof(double)));
  } else {
    pv->wait_seq = pv->sent_seq;     /* the update kernel's launch writes the words and this number behind them */
  }
  pv->sent_seq = 0.0;
  pv->rtr_valid = 0;
  return 0;
}
static int stopping_begin(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  if (stopping_queue(ecg, pv)) return 1;
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
  if (pv->bj_epoch != pa_bj_apply_epoch()) {
    /* the preconditioner was created again, or its coarse space set or cleared, since the capture: the graphs hold
     * the old launches and pointers (the entry that changed them has drained the stream), so capture anew */
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 6; ++b) { pa_rt_graph_free(pv->graph[a][b]); pv->graph[a][b] = NULL; pv->seen[a][b] = 0; }
    pv->bj_epoch = pa_bj_apply_epoch();
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
  int rc = preAlps_ECGIterate(ecg, rci_request) || stopping_queue(ecg, pv);
  if (seg_end(pv, 0, mode, rc)) return 1;
  PA_CHECK(pa_rt_event_record(pv->ev_res));
  mode = seg_begin(pv, 1);
  rc = (ecg->ortho_alg == ORTHOMIN ? preAlps_BlockJacobiApply(ecg->R, ecg->Z) : preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) ||
       preAlps_ECGIterate(ecg, rci_request) || preAlps_BlockOperator(ecg->P, ecg->AP);
  if (seg_end(pv, 1, mode, rc)) return 1;
  pv->phase = (pv->phase + 1) % 6;
  return stopping_end(ecg, pv, stop);
}

static int stopping_end(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* stop) {
  if (pv->wait_seq != 0.0) { if (wait_for_note(pv)) return 1; }
  else PA_CHECK(pa_rt_event_wait(pv->ev_res));
  double res2 = pv->h_pin[0];
  int info = (int)pv->h_pin[1];
  if (info != 0 && ecg->ortho_alg == ORTHOMIN) return PA_FAIL("ACHQR: dpotrf:\n ERROR: P^tAP is not spd!");
  ecg->res = sqrt(res2);
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
    *stop = (above && !nan && ecg->iter < ecg->maxIter && ecg->bs > 0) ? 0 : 1;
    return 0;
  }
  /* !(a > b) also stops on NaN, like the reference's comparison */
  if (ecg->res > ecg->normb * ecg->tol && ecg->iter < ecg->maxIter && ecg->bs > 0) *stop = 0;
  else *stop = 1;
  return 0;
}

int preAlps_ECGStoppingCriterion(preAlps_ECG_t* ecg, int* stop) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  if (!stop) return PA_FAIL(" wrong test 'stop != NULL'");
  double tg = pa_wtime();
  if (stopping_begin(ecg, pv)) return 1;
  if (stopping_end(ecg, pv, stop)) return 1;
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
  if (queue_group_norms(ecg, pv, defer ? pv->lazy_ptr : pv->d_res2)) return 1;
  TAC(PA_T_UPDATE, trsm_t);
  pv->rtr_valid = defer ? 1 : 2;
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
  if (queue_group_norms(ecg, pv, pv->d_res2)) return 1;
  TAC(PA_T_UPDATE, gemm_t);
  pv->rtr_valid = 2;
  pv->lazy_ptr = NULL;
  return 0;
}

/* The reference's "Swapping time" (ecg.c:521-523 / :358): without block-size
 * reduction all columns are live, so the copies become pointer rotations. */
static int shift_directions(preAlps_ECG_t* ecg, ecg_priv_t* pv, int ncopy) {
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
    if (pv->rtr_valid == 1 && pv->lazy_ptr && pv->lazy_ptr == pv->d_beta + cnt) {
      PA_CHECK(pa_k_finish32_trace(pv->d_bj_parts, from_bj, scratch, pv->d_beta, pv->d_rtr_part, pv->rtr_nblk, pv->ts, T,
                                   pv->lazy_ptr, pv->d_info));
      pv->rtr_valid = 2;
    } else {
      if (pv->rtr_valid == 1 && pv->lazy_ptr) {
        PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->lazy_ptr, pv->d_info, NULL));
        pv->rtr_valid = 2;
      }
      PA_CHECK(pa_k_finish32(pv->d_bj_parts, from_bj, scratch, 0, 0, pv->d_beta, NULL, NULL, NULL));
    }
  } else if (pv->rtr_valid == 1 && pv->lazy_ptr && pv->lazy_ptr == pv->d_beta + cnt) {
    /* the column sums fused_first_half left: summed by the same launch, into the slot behind beta */
    PA_CHECK(pa_k_gram_finish_trace(pv->m, pv->ts, pv->buf_av[0], a_hi > 0 ? pv->buf_av[1] : NULL, pv->buf_z,
                                    pv->d_partials, a_lo, a_hi, ecg->beta->info.n, pv->d_beta, ecg->beta->info.lda,
                                    pv->d_rtr_part, pv->rtr_nblk, T, pv->lazy_ptr, pv->d_info));
    pv->rtr_valid = 2;
  } else {
    if (pv->rtr_valid == 1 && pv->lazy_ptr) {     /* (beta not where expected: the norm by itself) */
      PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, pv->rtr_nblk, pv->ts, T, pv->lazy_ptr, pv->d_info, NULL));
      pv->rtr_valid = 2;
    }
    PA_CHECK(pa_k_gram_finish(pv->m, pv->ts, pv->buf_av[0], a_hi > 0 ? pv->buf_av[1] : NULL, pv->buf_z,
                              pv->d_partials, a_lo, a_hi, ecg->beta->info.n, pv->d_beta, ecg->beta->info.lda,
                              0, 0, NULL, NULL, NULL));
  }
  TAC(PA_T_GRAM, gemm_t);
  TIC(PA_T_COMM);
  {
    if (pv->rtr_valid == 2 && pv->lazy_ptr == pv->d_beta + cnt) {
      /* the norm of the new residual (and the Cholesky status) ride along; the update kernel
       * below passes them on to the pinned words the host reads (a copy here costs a launch and
       * 8 us of idle stream behind it);
       * several systems on several processes: their k local sums lie right behind the pair
       * (pa_k_group_norms_ride), ride in the same collective, and reach h_grp ahead of the event below */
      if (pa_allreduce(pv->d_beta, cnt + 2 + (pv->ride ? pv->nrhs : 0))) return 1;
      if (pv->ride) PA_CHECK(pa_rt_d2h_async(pv->h_grp, pv->lazy_ptr + 2, (size_t)pv->nrhs * sizeof(double)));
      note = pv->lazy_ptr;
      pv->rtr_valid = 0;
    } else {
      if (pa_allreduce(pv->d_beta, cnt)) return 1;
      if (pv->lazy_ptr && pv->rtr_valid == 2) {   /* (beta not where expected: reduce the norm by itself) */
        if (pa_allreduce(pv->lazy_ptr, pv->ride ? 2 + pv->nrhs : 1)) return 1;
        if (pv->ride) PA_CHECK(pa_rt_d2h_async(pv->h_grp, pv->lazy_ptr + 2, (size_t)pv->nrhs * sizeof(double)));
        PA_CHECK(pa_rt_d2h_async(pv->h_pin, pv->lazy_ptr, 2 * sizeof(double)));
        PA_CHECK(pa_rt_event_record(pv->ev_res));
        pv->wait_seq = 0.0;
        pv->rtr_valid = 0;
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
    if (shift_directions(ecg, pv, t)) return 1;
    request_gram_from_spmm(ecg, pv);
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
    if (!one_pass && shift_directions(ecg, pv, nrhs)) return 1;
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
    request_gram_from_spmm(ecg, pv);
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
  if (!pv->rtr_valid) PA_CHECK(pa_k_colnorm2(m, ts, pv->d_R, pv->d_rtr_part, &pv->rtr_nblk));
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
  return shift_directions(ecg, pv, ecg->bs);
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
  /* x = X * ones (ecg.c:674); the partial sums go through the free Z buffer */
  double* d_sol = pv->d_partials;
  size_t room = (size_t)pa_gram_max_blocks() * 2 * pv->ts * pv->ts;
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
 * only, as the other order does: leaving the library's loop ends the Gram request of the SpMM (leave_own_loop), so
 * that order forms the first alpha of the next call with pa_k_gram_finish, and so must this one to give the same
 * bits; a call therefore returns in the state "AP = A P is queued" of the RCI protocol (rci 0), as it always did. */
static int solve_first_applies(preAlps_ECG_t* ecg, ecg_priv_t* pv) {
  return g_own_loop > 0 && ecg->P->info.n == 4 && pv->ts == 4 && !pv->ride &&      /* (ride: several processes) */
         solve_first_rule(pv->solve_first, pa_world_size(), ecg->ortho_alg, ecg->bs_red, ecg->enlFac, pv->fuse,
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
  TIC(PA_T_UPDATE);
  PA_CHECK(pa_k_update_xrz(pv->m, pv->ts, t, pv->d_mu, pv->d_alpha, ecg->P->val, ecg->AP->val, pv->buf_v[1], pv->d_X,
                           pv->d_R, pv->buf_z, pv->d_rtr_part, &nb, pv->d_uu + (size_t)pv->uu_cur * T * T, pv->d_beta,
                           ecg->beta->info.lda, pv->d_uu + (size_t)(1 - pv->uu_cur) * T * T));
  TAC(PA_T_UPDATE, trsm_t);
  pv->rtr_nblk = nb;
  if (queue_group_norms(ecg, pv, NULL)) return 1;      /* (never pv->ride: solve_first_applies) */
  pv->uu_cur ^= 1;
  ecg->iter++;
  /* the norm of the new residual (and the Cholesky status) straight to the pinned words the host reads */
  pv->wait_seq = 0.0;
  if (pv->poll) { pv->wait_seq = (pv->seq += 1.0); pa_k_note_seq(pv->wait_seq); }
  PA_CHECK(pa_k_trace_finish(pv->d_rtr_part, nb, pv->ts, T, pv->d_res2, pv->d_info, pv->h_pin));
  if (!pv->poll) PA_CHECK(pa_rt_event_record(pv->ev_res));
  pv->rtr_valid = 0; pv->sent_seq = 0.0; pv->lazy_ptr = NULL;
  if (shift_directions(ecg, pv, t)) return 1;
  request_gram_from_spmm(ecg, pv);
  if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
  if (ahead && sf_queue_solve(ecg, pv)) return 1;
  ecg->tot_t += pa_wtime() - tg;
  return stopping_end(ecg, pv, stop);
}

/* The driver loop of examples/test_ecg_prealps_op.c:203-223 (fused:
 * examples/test_ecg_bench_fused.c:243-259). */
typedef struct {      /* what preAlps_ECGSolveMulti adds to the arguments of preAlps_ECGSolve; nrhs = 0: the latter */
  int nrhs, ldrhs, ldsol;
  double* sys_hist; double* sys_normb;
  const double* x0; int ldx0; double* sys_res0;   /* ... and preAlps_ECGSolveGuess to those; x0 = NULL: the former */
  /* ... and preAlps_ECGSolveSystem: the caller's arrays (sys->b, sys->x0: the rows in the caller's order and units), the
   * solution and the final norms in the caller's units; sys = NULL: one of the others */
  const sys_in_t* sys; double* sys_x; int sys_ldx; double* sys_res;
} multi_args_t;
static int ecg_solve_loop(preAlps_ECG_t* ecg, double* rhs, double* sol, double* res_hist, int* bs_hist,
                          int max_hist, int* n_hist, const multi_args_t* mu);
static int finish_system(preAlps_ECG_t* ecg, const multi_args_t* mu, int as_x0);
static void leave_own_loop(void) {
  if (--g_own_loop == 0) { pa_k_spmm_gram_disarm(NULL); pa_k_bj_gram_disarm(NULL); }
}
int preAlps_ECGSolve(preAlps_ECG_t* ecg, double* rhs, double* sol, double* res_hist, int* bs_hist,
                     int max_hist, int* n_hist) {
  ++g_own_loop;
  const multi_args_t one = {0, 0, 0, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL};
  int rc = ecg_solve_loop(ecg, rhs, sol, res_hist, bs_hist, max_hist, n_hist, &one);
  leave_own_loop();
  return rc;
}
/* preAlps_ECGInitializeMulti, the loop of preAlps_ECGSolve (the same body, so the same branch of it for the same
 * settings), preAlps_ECGFinalizeMulti. */
int preAlps_ECGSolveMulti(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, double* sol, int ldsol,
                          double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                          int max_hist, int* n_hist) {
  const pa_operator_info_t* op = pa_operator_info();
  if (nrhs < 1) return PA_FAIL("nrhs = %d: at least one right-hand side is needed", nrhs);
  if (sol && op && ldsol < op->m) return PA_FAIL("ldsol = %d is smaller than the %d local rows", ldsol, op->m);
  const multi_args_t mu = {nrhs, ldrhs, ldsol, sys_hist, sys_normb, NULL, 0, NULL, NULL, NULL, 0, NULL};
  ++g_own_loop;
  int rc = ecg_solve_loop(ecg, (double*)rhs, sol, res_hist, bs_hist, max_hist, n_hist, &mu);
  leave_own_loop();
  return rc;
}
/* The same around preAlps_ECGInitializeGuess; x0 = NULL: preAlps_ECGSolveMulti (sys_res0 then receives ||b_j||).
 * A guess under which every system already meets its threshold comes back as the solution, with no iteration. */
int preAlps_ECGSolveGuess(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, const double* x0, int ldx0,
                          double* sol, int ldsol, double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                          double* sys_res0, int max_hist, int* n_hist) {
  const pa_operator_info_t* op = pa_operator_info();
  if (nrhs < 1) return PA_FAIL("nrhs = %d: at least one right-hand side is needed", nrhs);
  if (sol && op && ldsol < op->m) return PA_FAIL("ldsol = %d is smaller than the %d local rows", ldsol, op->m);
  const multi_args_t mu = {nrhs, ldrhs, ldsol, sys_hist, sys_normb, x0, ldx0, sys_res0, NULL, NULL, 0, NULL};
  ++g_own_loop;
  int rc = ecg_solve_loop(ecg, (double*)rhs, sol, res_hist, bs_hist, max_hist, n_hist, &mu);
  leave_own_loop();
  return rc;
}
/* The end of a system solve: the recurrence residual norms in the caller's units (one pa_k_sys_norms on R, whichever
 * metric stopped the loop: with the caller's metric the launch and the data of the last stopping test, so the same
 * bits), the solutions scattered into the caller's order and units -- as_x0: the guess itself, copied -- and the
 * solver released.  Returns after the stream has drained. */
static int finish_system(preAlps_ECG_t* ecg, const multi_args_t* mu, int as_x0) {
  ecg_priv_t* pv = priv_of(ecg);
  if (!pv) return PA_FAIL("solver not initialised");
  const pa_operator_info_t* op = pa_operator_info();
  const sys_in_t* in = mu->sys;
  const int m = pv->m, k = pv->nrhs > 1 ? pv->nrhs : 1, s = pv->sgrp;
  const size_t mm = (size_t)(m > 0 ? m : 1);
  const int* d_src = NULL; const double* d_dl = NULL;
  double* tmp = NULL;
  int nb = 0;
  int rc = !op || pa_operator_system_map(&d_src, &d_dl);
  if (!rc && (pa_k_sys_norms(m, pv->ts, k, s, ecg->R->val, d_dl, pv->d_sys_part, &nb) ||
              pa_k_group_norms(pv->d_sys_part, nb, pv->ts, k, 1, pv->d_grp, pv->h_grp)))
    rc = PA_FAIL("%s", pa_rt_error());
  if (!rc && as_x0) {
    for (int j = 0; j < k && !rc; ++j) {
      if (in->device) rc = pa_rt_d2d(mu->sys_x + (size_t)j * mu->sys_ldx, in->x0 + (size_t)j * in->ldx0, (size_t)m * sizeof(double));
      else memcpy(mu->sys_x + (size_t)j * mu->sys_ldx, in->x0 + (size_t)j * in->ldx0, (size_t)m * sizeof(double));
    }
    if (rc) rc = PA_FAIL("%s", pa_rt_error());
  } else if (!rc) {
    double* d_out = mu->sys_x;
    int ld = mu->sys_ldx;
    if (!in->device) {
      tmp = (double*)pa_rt_malloc(mm * k * sizeof(double));
      if (!tmp) rc = PA_FAIL("buffers for %d solutions: %s", k, pa_rt_error());
      d_out = tmp; ld = m;
    }
    if (!rc && pa_k_sys_scatter(m, pv->ts, k, s, pv->d_X, d_src, d_dl, d_out, ld)) rc = PA_FAIL("%s", pa_rt_error());
    /* (d_out holds the caller's rows: row src[i] of column j at src[i] + j*m, the order of the caller's x) */
    for (int j = 0; tmp && j < k && !rc; ++j)
      if (pa_rt_d2h(mu->sys_x + (size_t)j * mu->sys_ldx, tmp + (size_t)j * m, (size_t)m * sizeof(double)))
        rc = PA_FAIL("%s", pa_rt_error());
  }
  if (!rc && pa_rt_sync()) rc = PA_FAIL("%s", pa_rt_error());
  for (int j = 0; j < k && !rc && mu->sys_res; ++j) mu->sys_res[j] = sqrt(pv->h_grp[j]);
  pa_rt_free(tmp);
  _preAlps_ECGFree(ecg);
  return rc;
}

/* preAlps_ECGSolveGuess around the gather and the scatter: A x = b as the caller stated it (one process: N = m). */
int preAlps_ECGSolveSystem(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, const double* x0, int ldx0, double* x,
                           int ldx, int flags, double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                           double* sys_res, int max_hist, int* n_hist) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built before the solver");
  if (!ecg || !b || !x) return PA_FAIL(" wrong test 'ecg != NULL && b != NULL && x != NULL'");
  if (nrhs < 1) return PA_FAIL("nrhs = %d: at least one right-hand side is needed", nrhs);
  if (flags & ~(PREALPS_SYS_DEVICE | PREALPS_SYS_STOP_ORIGINAL)) return PA_FAIL("flags = %d holds unknown bits", flags);
  if (ldb < op->N) return PA_FAIL("ldb = %d is smaller than the %d rows of the matrix", ldb, op->N);
  if (x0 && ldx0 < op->N) return PA_FAIL("ldx0 = %d is smaller than the %d rows of the matrix", ldx0, op->N);
  if (ldx < op->N) return PA_FAIL("ldx = %d is smaller than the %d rows of the matrix", ldx, op->N);
  const sys_in_t in = {b, ldb, x0, ldx0, (flags & PREALPS_SYS_DEVICE) != 0, (flags & PREALPS_SYS_STOP_ORIGINAL) != 0, 0};
  const multi_args_t mu = {nrhs, 0, 0, sys_hist, sys_normb, NULL, 0, NULL, &in, x, ldx, sys_res};
  ++g_own_loop;
  int rc = ecg_solve_loop(ecg, NULL, NULL, res_hist, bs_hist, max_hist, n_hist, &mu);
  leave_own_loop();
  return rc;
}

/* A fresh ||b_j - A x_j|| and ||b_j|| in the caller's units: one start from the guess x at s = 1 on a temporary solver
 * of width nrhs -- the gather, the library's own product, R0 -- pa_k_sys_norms on its R0, and a free.  No
 * preconditioner is needed, and nothing of an iteration is queued. */
int preAlps_OperatorSystemResiduals(int nrhs, const double* b, int ldb, const double* x, int ldx, int flags, double* res,
                                    double* normb) {
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return PA_FAIL("the operator must be built first");
  if (!b || !x) return PA_FAIL(" wrong test 'b != NULL && x != NULL'");
  if (nrhs < 1 || nrhs > 16)
    return PA_FAIL("nrhs = %d: between 1 and 16 systems at a time (what the per-system arrays of a solver hold)", nrhs);
  if (flags & ~PREALPS_SYS_DEVICE) return PA_FAIL("flags = %d: only PREALPS_SYS_DEVICE applies here", flags);
  if (ldb < op->N) return PA_FAIL("ldb = %d is smaller than the %d rows of the matrix", ldb, op->N);
  if (ldx < op->N) return PA_FAIL("ldx = %d is smaller than the %d rows of the matrix", ldx, op->N);
  preAlps_ECG_t e;
  memset(&e, 0, sizeof(e));
  e.globPbSize = op->N; e.locPbSize = op->m; e.enlFac = nrhs; e.maxIter = 1; e.tol = 1e-5;
  e.ortho_alg = ORTHODIR; e.bs_red = NO_BS_RED;
  const sys_in_t in = {b, ldb, x, ldx, (flags & PREALPS_SYS_DEVICE) != 0, 1, 1};
  int rci = 0;
  if (start_systems(__func__, &e, nrhs, NULL, 0, x, ldx, &rci, &in)) return 1;
  ecg_priv_t* pv = priv_of(&e);
  for (int j = 0; j < nrhs; ++j) {
    if (res) res[j] = pv->sys_res[j];
    if (normb) normb[j] = pv->sys_normb[j];
  }
  _preAlps_ECGFree(&e);
  return 0;
}
/* one entry of the histories after a stopping test */
static void record_hist(preAlps_ECG_t* ecg, const multi_args_t* mu, double* res_hist, int* bs_hist, int max_hist,
                        int nh) {
  if (nh >= max_hist) return;
  if (res_hist) { res_hist[nh] = ecg->res; if (bs_hist) bs_hist[nh] = ecg->bs; }
  if (mu->nrhs > 0 && mu->sys_hist) {
    ecg_priv_t* pv = priv_of(ecg);
    for (int j = 0; j < mu->nrhs; ++j)
      mu->sys_hist[nh + (size_t)j * max_hist] = (pv && (pv->nrhs > 1 || pv->metric)) ? pv->sys_res[j] : ecg->res;
  }
}
static int ecg_solve_loop(preAlps_ECG_t* ecg, double* rhs, double* sol, double* res_hist, int* bs_hist,
                          int max_hist, int* n_hist, const multi_args_t* mu) {
  int rci = 0, stop = 0, nh = 0;
  if (mu->sys) {
    double g0[16], nb[16];
    int live = mu->sys->x0 == NULL;
    if (start_systems("preAlps_ECGSolveSystem", ecg, mu->nrhs, NULL, 0, mu->sys->x0, mu->sys->ldx0, &rci, mu->sys)) return 1;
    if (preAlps_ECGSystemResiduals(ecg, g0, nb)) return 1;
    for (int j = 0; j < mu->nrhs; ++j) {
      if (mu->sys_normb) mu->sys_normb[j] = nb[j];
      if (g0[j] > nb[j] * ecg->tol) live = 1;
    }
    if (!live) {
      /* every system meets its threshold, in the metric of the test, as it stands: x0 is the answer, bit for bit */
      if (n_hist) *n_hist = 0;
      return finish_system(ecg, mu, 1);
    }
  } else if (mu->nrhs > 0 && mu->x0) {
    double g0[16], nb[16];
    int live = 0;
    if (preAlps_ECGInitializeGuess(ecg, mu->nrhs, rhs, mu->ldrhs, mu->x0, mu->ldx0, &rci)) return 1;
    if (preAlps_ECGSystemResiduals(ecg, g0, nb)) return 1;
    for (int j = 0; j < mu->nrhs; ++j) {
      if (mu->sys_normb) mu->sys_normb[j] = nb[j];
      if (mu->sys_res0) mu->sys_res0[j] = g0[j];
      if (g0[j] > nb[j] * ecg->tol) live = 1;
    }
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
          if (stopping_begin(ecg, pv)) return 1;
          if (preAlps_ECGIterate(ecg, &rci)) return 1;
          if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
        } else if (pv->lazy_stop && pv->lazy_ptr) {
          /* several processes: the norm travels with the beta all-reduce of the second half;
           * the half-step and the product queued before the decision are unused after a stop */
          if (ecg->ortho_alg == ORTHOMIN) { if (preAlps_BlockJacobiApply(ecg->R, ecg->Z)) return 1; }
          else if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
          if (preAlps_ECGIterate(ecg, &rci)) return 1;
          if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
        } else {
          if (stopping_begin(ecg, pv)) return 1;
          if (ecg->ortho_alg == ORTHOMIN) { if (preAlps_BlockJacobiApply(ecg->R, ecg->Z)) return 1; }
          else if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
        }
        if (stopping_end(ecg, pv, &stop)) return 1;
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
  if (mu->sys) return finish_system(ecg, mu, 0);
  if (sol) return mu->nrhs > 0 ? preAlps_ECGFinalizeMulti(ecg, sol, mu->ldsol) : preAlps_ECGFinalize(ecg, sol);
  return 0;
}

/* Advance the driver loop (examples/test_ecg_prealps_op.c:208-221) by nsteps full
 * iterations, restarting from the same rhs (as after preAlps_ECGInitialize) whenever the
 * stopping test fires; what bench.py times. */
static int ecg_advance_loop(preAlps_ECG_t* ecg, double* rhs, int* rci_request, int nsteps, int* restarts,
                            int* last_iters, double* last_res);
int preAlps_ECGAdvance(preAlps_ECG_t* ecg, double* rhs, int* rci_request, int nsteps, int* restarts,
                       int* last_iters, double* last_res) {
  ecg_priv_t* pvm = priv_of(ecg);
  if (pvm && pvm->guess)
    return PA_FAIL("the solver was started from an initial guess: a restart from the right-hand side alone would drop "
                   "x0 (use preAlps_ECGSolveGuess or the caller's own loop, or _preAlps_ECGReset for a cold start)");
  if (pvm && pvm->nrhs > 1)
    return PA_FAIL("the solver holds %d systems: restarts from one right-hand side are not defined for it "
                   "(use preAlps_ECGSolveMulti or the caller's own loop)", pvm->nrhs);
  ++g_own_loop;
  int rc = ecg_advance_loop(ecg, rhs, rci_request, nsteps, restarts, last_iters, last_res);
  leave_own_loop();
  return rc;
}
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
      if (*rci_request == 1) {
        if (restarts) ++*restarts;
        if (last_iters) *last_iters = ecg->iter;
        if (last_res) *last_res = ecg->res;
        if (_preAlps_ECGReset(ecg, rhs, rci_request)) return 1;
        if (preAlps_BlockJacobiApply(ecg->R, ecg->P)) return 1;
      }
    }
    return 0;
  }
  {
    ecg_priv_t* pvg = priv_of(ecg);
    if (pvg && pvg->use_graphs && *rci_request == 0) {
      while (done < nsteps) {
        if (graph_iteration(ecg, pvg, rci_request, &stop)) return 1;
        ++done;
        if (stop == 1) {
          if (restarts) ++*restarts;
          if (last_iters) *last_iters = ecg->iter;
          if (last_res) *last_res = ecg->res;
          if (_preAlps_ECGReset(ecg, rhs, rci_request)) return 1;
          if (preAlps_BlockJacobiApply(ecg->R, ecg->P)) return 1;
          if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
        }
      }
      return 0;
    }
    if (pvg && *rci_request == 0 && solve_first_applies(ecg, pvg)) {
      while (done < nsteps) {
        if (solve_first_step(ecg, pvg, done + 1 < nsteps, &stop)) return 1;
        ++done;
        if (stop == 1) {
          if (restarts) ++*restarts;
          if (last_iters) *last_iters = ecg->iter;
          if (last_res) *last_res = ecg->res;
          if (_preAlps_ECGReset(ecg, rhs, rci_request)) return 1;
          if (preAlps_BlockJacobiApply(ecg->R, ecg->P)) return 1;
          if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
        }
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
        if (early) { pv->z_ready = 0; if (stopping_begin(ecg, pv)) return 1; }
        else if (ecg->ortho_alg == ORTHOMIN) { if (preAlps_BlockJacobiApply(ecg->R, ecg->Z)) return 1; }
        else if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
        if (preAlps_ECGIterate(ecg, rci_request)) return 1;
        if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
      } else {
        if (stopping_begin(ecg, pv)) return 1;
        if (ecg->ortho_alg == ORTHOMIN) { if (preAlps_BlockJacobiApply(ecg->R, ecg->Z)) return 1; }
        else if (preAlps_BlockJacobiApply(ecg->AP, ecg->Z)) return 1;
      }
      if (stopping_end(ecg, pv, &stop)) return 1;
      if (lazy && stop != 1) ++done;
      if (stop == 1) {
        if (restarts) ++*restarts;
        if (last_iters) *last_iters = ecg->iter;
        if (last_res) *last_res = ecg->res;
        if (_preAlps_ECGReset(ecg, rhs, rci_request)) return 1;
        if (preAlps_BlockJacobiApply(ecg->R, ecg->P)) return 1;
        if (preAlps_BlockOperator(ecg->P, ecg->AP)) return 1;
        ++done;
        continue;
      }
    }
  }
  return 0;
}
