/*
 * ecg_priv.h -- the state of an ECG solver and what the units of the solver share:
 *   ecg.c        pool, reset, stopping test, the RCI iteration halves, wrap-up
 *   ecg_start.c  the start of one or several systems (guess, caller's units, several ranks) and their finish
 *   ecg_loops.c  the library's own driver loops (graphs, solve first, preAlps_ECGSolve* / preAlps_ECGAdvance)
 *   ecg_plan.c   the pool layout and the switch decisions, pure host arithmetic
 */
#ifndef PA_ECG_PRIV_H
#define PA_ECG_PRIV_H

#include "pa_host.h"
#include "ecg_plan.h"
#include "ecg_energy.h"

#define PA_ECG_MAGIC 0x45434731u

/* The reference brackets every BLAS / MPI call with MPI_Wtime (ecg.c:316-320 ...).  Launches
 * are asynchronous here, so the host clock only sees the enqueue; with preAlps_hip_timing(1)
 * the phase's hipEvent pair is read instead (one stream sync per phase) and the timer fields
 * of preAlps_ECG_t hold device time, which is what preAlps_ECGPrint then reports. */
#define TIC(key) do { pa_time_begin(key); t0 = pa_wtime(); } while (0)
#define TAC(key, field) \
  do { double d_ = pa_time_end(key); ecg->field += d_ >= 0.0 ? d_ : pa_wtime() - t0; } while (0)

/* What is left of the column sums of R^2 in d_rtr_part (rtr_valid). */
enum {
  RTR_NONE = 0,       /* nothing is left */
  RTR_COLUMN_SUMS,    /* the column sums are left by the update and the norm is not summed yet */
  RTR_SUMMED,         /* summed, and on one process already on its way to the pinned words */
  RTR_ON_DEVICE       /* summed on the device, not on the host yet */
};

typedef struct {
  unsigned magic;
  int ts, T, m;
  pa_ecg_pool_t lay;  /* where every region of the pool lies (pa_ecg_pool_layout) */
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
  int lazy_stop;      /* several processes: the residual norm rides on the beta all-reduce (see pa_ecg_switches) */
  double* lazy_ptr;   /* where the first half left [res2, potrf status] for that */
  /* graphs (driver loops of this library): an iteration is two segments -- 0: the first half up to
   * the residual norm, 1: preconditioner apply + second half + product -- and the panel pointers
   * rotate with period 6 (three P slots x two AP slots), so there are 2 x 6 graphs */
  int use_graphs;
  /* solve_first: the library's own loops run an Orthodir iteration with the block solve before the update (see
   * solve_first_step; PREALPS_ECG_SOLVE_FIRST, read at reset).  sf_ready: the block solve and the finish of the
   * next iteration are queued behind its product (only inside one call of those loops, see solve_first_step). */
  int solve_first, sf_ready;
  /* X every second row pass (solve_first_step only; PREALPS_ECG_X_DEFER, read at reset; the rule: pa_ecg_x_mode).
   * x_pending: the last row pass left X as it was and owes it x += (p U^-1) alpha -- that P is the raw panel in
   * buf_v[1] now, its factor is d_uu's previous slot, and its alpha is in the same slot of d_akeep (an allocation of
   * its own, two t x t blocks indexed like d_uu: the next finish overwrites d_alpha).  INVARIANT: nothing is owed
   * whenever anything but the next row pass may touch X -- pa_ecg_flush_x pays on a stop, and is called again, for
   * nothing, before every reader of X and on every way out of the library's loops. */
  int x_defer, x_pending;
  double* d_akeep;
  int phase;          /* iterations since the last reset, mod 6 */
  void* graph[2][6];
  unsigned char seen[2][6];
  int bj_epoch;       /* pa_bj_apply_epoch() the graphs were captured under */
  int op_epoch;       /* pa_operator_plan_epoch() likewise */
  /* Several right-hand sides (preAlps_ECGInitializeMulti): nrhs systems of sgrp = enlFac / nrhs columns each, system
   * j in the columns j*sgrp .. j*sgrp + sgrp - 1.  nrhs <= 1: one system, nothing below is used.  Every launch that
   * leaves the column sums of R^2 in d_rtr_part is followed by pa_k_group_norms (pa_ecg_queue_group_norms), which leaves
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
  /* The caller's metric on several processes (ride_sys; a preAlps_hip_loopback shard of such a group too): pa_k_sys_norms
   * leaves this process's share in d_sys_part, and pa_k_sys_norms_ride folds it behind the pair at grp_dst exactly
   * where ride puts the sums of several systems: [norm^2, status | g_0^2 .. g_nrhs-1^2], nrhs >= 1 words behind the
   * pair, in the same collective.  Every site that reads `ride` reads pa_ecg_rides instead. */
  int ride_sys;
  /* The energy-norm drops (preAlps_ECGSolveSystemEnergy; ecg_energy.h).  energy != NULL: every launch that updates X
   * and R (fused_update, update_iterate, the row pass of solve_first_step) is followed by pa_k_energy_drops on d_alpha,
   * which at that point holds the coefficients of this iteration's A-orthonormal directions and is next written by the
   * next iteration's finish; the k drops go to d_drop and to the pinned words h_drop (both allocated by
   * pa_ecg_energy_enable, not in the pool), ahead of whatever carries the norm to the host, and the stopping test
   * pushes them into the tracker, which belongs to the entry.  energy_stop: the test stops on the tracker's rule
   * instead of the residual norms.  Polling and graphs are off, as for several systems: the drops may be queued behind
   * the launch that writes the polled word.  pa_ecg_reset_state ends the request. */
  pa_energy_t* energy;
  int energy_stop;
  double* d_drop; double* h_drop;
} ecg_priv_t;
static inline int pa_ecg_rides(const ecg_priv_t* pv) { return pv->ride || pv->ride_sys; }

static inline ecg_priv_t* priv_of(preAlps_ECG_t* ecg) {
  if (!ecg || !ecg->iwork) return NULL;
  int T = ecg->enlFac;
  int skip = (T + 3) & ~3; /* iwork[0..T) stays the pivot array of the reference */
  ecg_priv_t* p = (ecg_priv_t*)(ecg->iwork + skip);
  return p->magic == PA_ECG_MAGIC ? p : NULL;
}

/* The caller's own system (preAlps_ECGSolveSystem, preAlps_OperatorSystemResiduals): b and x0 hold the rows in the order
 * and units of the matrix the operator was built from, on the host or (device) on the device.  pa_k_sys_gather fills
 * the staging arrays d_B / d_X0 that the host path uploads into -- b' = dl * b[src], x0' = x0[src] / dl -- and leaves
 * the caller's ||b_j||^2; what follows the uploads is the same code.  metric: the stopping test is the caller's;
 * probe: only the start's norms are wanted, so a system that starts at exactly zero is no refusal.
 * Several processes: the arrays are still the caller's global ones; a rank reads and writes the rows it owns.  ldx: the
 * leading dimension of the solution array (0: there is none), kept here because on several processes the verdicts on
 * the leading dimensions are agreed on by the start instead of being returned at once. */
typedef struct { const double* b; int ldb; const double* x0; int ldx0; int device, metric, probe; int ldx; } sys_in_t;

typedef struct {      /* what preAlps_ECGSolveMulti adds to the arguments of preAlps_ECGSolve; nrhs = 0: the latter */
  int nrhs, ldrhs, ldsol;
  double* sys_hist; double* sys_normb;
  const double* x0; int ldx0; double* sys_res0;   /* ... and preAlps_ECGSolveGuess to those; x0 = NULL: the former */
  /* ... and preAlps_ECGSolveSystem: the caller's arrays (sys->b, sys->x0: the rows in the caller's order and units), the
   * solution and the final norms in the caller's units; sys = NULL: one of the others */
  const sys_in_t* sys; double* sys_x; int sys_ldx; double* sys_res;
  /* ... and preAlps_ECGSolveSystemRefined: gate (NULL: none) is asked once the start's norms are known and a system is
   * above its threshold -- g0[j], nb[j]: the start residual and ||b_j|| of system j in the metric of the test --
   * and a nonzero answer ends the solve there as a converged guess ends it: x0 comes back as x, after no iteration.
   * sys_hist_ld: the leading dimension of sys_hist where it is not max_hist (0: it is). */
  int (*gate)(void* ctx, int nrhs, const double* g0, const double* nb); void* gate_ctx;
  int sys_hist_ld;
  /* ... and preAlps_ECGSolveSystemEnergy: the tracker the drops of every iteration are pushed into (NULL: none are
   * formed), and whether its rule is the stopping test */
  pa_energy_t* energy; int energy_stop;
} multi_args_t;

/* ---- ecg.c ---- */
int pa_ecg_in_own_loop(void);          /* > 0 inside preAlps_ECGSolve* / preAlps_ECGAdvance (g_own_loop) */
void pa_ecg_enter_own_loop(void);
void pa_ecg_leave_own_loop(void);      /* the last one out ends the Gram requests of the SpMM and the block solve */
int pa_ecg_reset_state(preAlps_ECG_t* ecg, ecg_priv_t* pv, int nrhs, int guess, int metric);
void pa_ecg_reset_done(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* rci_request);
void pa_ecg_request_gram_from_spmm(preAlps_ECG_t* ecg, ecg_priv_t* pv);
int pa_ecg_queue_group_norms(preAlps_ECG_t* ecg, ecg_priv_t* pv, double* dst);
int pa_ecg_stopping_queue(preAlps_ECG_t* ecg, ecg_priv_t* pv);
int pa_ecg_stopping_begin(preAlps_ECG_t* ecg, ecg_priv_t* pv);
int pa_ecg_stopping_end(preAlps_ECG_t* ecg, ecg_priv_t* pv, int* stop);
int pa_ecg_shift_directions(preAlps_ECG_t* ecg, ecg_priv_t* pv, int ncopy);
void pa_ecg_x_owed(ecg_priv_t* pv);                        /* a row pass skipped X: sets x_pending, counts */
int pa_ecg_flush_x(preAlps_ECG_t* ecg, ecg_priv_t* pv);    /* pays what is owed to X, if anything (pa_k_flush_x) */
int pa_ecg_energy_enable(preAlps_ECG_t* ecg, ecg_priv_t* pv, pa_energy_t* tracker, int stop);
int pa_ecg_queue_energy(preAlps_ECG_t* ecg, ecg_priv_t* pv);   /* the drops of the update just queued; nothing without a tracker */
/* ---- ecg_loops.c ---- */
int pa_ecg_solve_system_from(const char* who, preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, const double* x0,
                             int ldx0, double* x, int ldx, int flags, double* res_hist, int* bs_hist, double* sys_hist,
                             double* sys_normb, double* sys_res, double* sys_res0, int max_hist, int* n_hist);
/* ---- ecg_start.c ---- */
int pa_ecg_start_systems(const char* who, preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs,
                         const double* x0, int ldx0, int* rci_request, const sys_in_t* sys);
int pa_ecg_finish_system(preAlps_ECG_t* ecg, const multi_args_t* mu, int as_x0);

#endif
