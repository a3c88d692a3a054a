/*
 * ecg_plan.c -- the pool layout and the switch decisions of an ECG solver (see ecg_plan.h).
 */
#include "ecg_plan.h"

static size_t take(size_t* w, size_t n, int present) {
  if (!present) return PA_ECG_ABSENT;
  const size_t at = *w;
  *w += n;
  return at;
}

/* pool: same order as the reference (V, AV, Z, R, X, then the small blocks);
 * Orthomin needs no P_prev / AP_prev slots (ecg.c:55-61) */
void pa_ecg_pool_layout(const pa_ecg_pool_in_t* in, pa_ecg_pool_t* out) {
  const size_t T2 = (size_t)in->T * in->T, ts = (size_t)in->ts, G = (size_t)in->G, S = (size_t)in->S;
  const size_t panel = (size_t)(in->m > 0 ? in->m : 1) * ts;
  const int prev = in->ortho_alg != PA_ECG_ORTHOMIN;
  size_t w = 0;
  out->v[0] = take(&w, panel, 1);
  out->v[1] = take(&w, panel, prev);
  out->av[0] = take(&w, panel, 1);
  out->av[1] = take(&w, panel, prev);
  out->z = take(&w, panel, 1);
  out->r = take(&w, panel, 1);
  out->x = take(&w, panel, 1);
  out->F = take(&w, 5 * T2, 1);
  out->alpha = out->F; out->beta = out->F + T2; out->mu = out->F + 3 * T2; out->rtr = out->F + 4 * T2;
  out->q = take(&w, 2 * T2, 1);
  out->res2 = take(&w, 24, 1);
  out->uu = take(&w, 2 * T2, 1);
  out->partials = take(&w, G * 2 * ts * ts, 1);
  out->rtr_part = take(&w, G * ts, 1);
  /* T = 4: the library's SpMM can form [AP | R]^T P while it computes AP (one block per workgroup) ... */
  out->spmm_parts = take(&w, ((size_t)in->spmm_cap + S) * 32, in->spmm_cap > 0);
  /* ... and the library's block solve beta = [AP | AP_prev]^T Z while Z is still in its registers (Orthodir) */
  out->bj_parts = take(&w, ((size_t)in->bj_cap + S) * 32, in->bj_cap > 0);
  out->grp = take(&w, 48, 1);
  out->sys_part = take(&w, G * ts, 1);
  out->pool_doubles = w;
}

void pa_ecg_switches(const pa_ecg_switch_in_t* in, pa_ecg_switch_t* out) {
  const int several = in->nrhs > 1 || in->guess || in->metric;
  out->rotate = in->bs_red == PA_ECG_NO_BS_RED;     /* NO_BS_RED: rotate pointers instead of copying */
  out->fuse = in->fuse;
  out->lazy_norm = in->fuse && in->ortho_alg == PA_ECG_ORTHODIR && in->lazy_norm;
  /* (a loopback shard of a group of ONE is a single process in every branch of the iteration -- the world size is
   * what they read -- and has nothing to reduce: it keeps pa_k_group_norms and the pinned mirror) */
  out->ride = in->nrhs > 1 && !in->metric && in->world > 1;
  /* the caller's metric on several processes: its sums are this process's share too, and ride the same way */
  out->ride_sys = in->metric && in->world > 1;
  /* With more than one process every collective costs tens of microseconds.  The norm of the
   * new residual is only needed for the stopping decision, so the driver loops of this library
   * (preAlps_ECGSolve / ECGAdvance) let it travel with the beta all-reduce of the same
   * iteration and decide one half-step later; the last half-step is then simply unused.  The
   * RCI entry preAlps_ECGStoppingCriterion keeps working (it reduces the norm by itself).
   * One process: the same order saves the launch that sums the norm (it is summed with beta):
   * 2-3 us per iteration (in-process A/B), so it is the default there too; PREALPS_ECG_LAZY_STOP=0
   * decides right after the update, as the reference does. */
  out->lazy_stop = in->fuse && in->bs_red == PA_ECG_NO_BS_RED && in->ortho_alg != PA_ECG_ORTHODIR_FUSED &&
                   in->enlFac >= 2 && in->lazy_stop;
  /* graphs (opt-in: preAlps_hip_graphs(1) or PREALPS_ECG_GRAPH=1): one process, or the one-shard
   * rehearsal of preAlps_hip_loopback, whose sums are free, so the stopping test need not ride on one;
   * =2 forces them for any process group (the hooks must then be capturable: RCCL is, host-staged ones
   * are not).  Off by default because they measure SLOWER on this stack: 436.5 us per iteration against
   * 423.2 us with plain launches on the headline problem (same box, 200 iterations each; ROCm 7.2 puts
   * more idle time between the nodes of a graph than between launches queued on a stream).
   * Several systems: the group launch is not part of the captured segments; a start from a guess: as for several
   * systems, whatever nrhs; the caller's metric: its two launches are not part of the segments either. */
  const int want = several ? 0 : in->graphs;
  const int group_ok = in->world == 1 || in->loopback || want == 2;
  out->use_graphs = want && group_ok && out->rotate && out->fuse && in->ortho_alg != PA_ECG_ORTHODIR_FUSED &&
                    !in->timing;
  if (out->use_graphs) out->lazy_stop = 0;
  /* the residual norm reaches the host through two pinned words a kernel writes; a third word behind
   * them (a sequence number) lets the host poll for them instead of waiting for an event recorded in the
   * stream.  Default with several processes, where it measures 5 us per iteration faster (one-shard
   * rehearsal: 112.5 against 117.8 us); one process: no difference (the 6 us bubble the event leaves
   * behind k_trace_finish reappears behind the block solve), so the event stays.  PREALPS_ECG_POLL=0 / 1
   * forces; graphs replay fixed arguments and keep the event.
   * Several systems: the per-system sums may be queued behind the launch that writes the polled word, so the
   * host waits for the event behind both. */
  out->poll = (in->poll >= 0 ? in->poll != 0 : in->world > 1) && !out->use_graphs && !several;
}

/* Where the order of solve_first_step applies (the switch on): one process, Orthodir without block-size reduction,
 * the two-pass first half with lazy normalisation and the lazy stopping test, 4 columns, the Gram blocks left behind
 * by the block solve and by the SpMM, no graphs.  Everything else keeps the order of preAlps_ECGIterate. */
int pa_ecg_solve_first_rule(int on, int nprocs, int ortho_alg, int bs_red, int enlFac, int fuse, int lazy_norm,
                            int lazy_stop, int bj_gram, int spmm_gram, int graphs) {
  return on && nprocs == 1 && ortho_alg == PA_ECG_ORTHODIR && bs_red == PA_ECG_NO_BS_RED && enlFac == 4 && fuse &&
         lazy_norm && lazy_stop && bj_gram && spmm_gram && !graphs;
}

int pa_ecg_x_mode(int on, int pending, int another_step_follows) {
  if (pending) return PA_ECG_X_BOTH;      /* (whatever the switch says now: a debt is paid) */
  return on && another_step_follows ? PA_ECG_X_SKIP : PA_ECG_X_EVERY;
}
