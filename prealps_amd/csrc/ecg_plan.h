/*
 * ecg_plan.h -- what a solver of ecg.c is laid out as and which branches of the iteration it takes, as plain
 * host arithmetic (ecg_plan.c): the one statement of the device pool's layout and the one table of the switch
 * decisions of a reset.  No device call, no environment, no globals: everything the rules depend on is passed
 * in, so the unit runs under a host sanitizer and in tests without a GPU (tests/test_ecg_plan_cpu.py).
 * ecg.c allocates and carves the pool from the offsets and copies the decisions into its state.
 */
#ifndef PA_ECG_PLAN_H
#define PA_ECG_PLAN_H

#include <stddef.h>

/* the values of preAlps_ECG_Ortho_Alg_t / preAlps_ECG_Block_Size_Red_t (preAlps_abi.h; ecg.c asserts the match) */
enum { PA_ECG_ORTHOMIN = 0, PA_ECG_ORTHODIR = 1, PA_ECG_ORTHODIR_FUSED = 2 };
enum { PA_ECG_ADAPT_BS = 0, PA_ECG_NO_BS_RED = 1 };

#define PA_ECG_ABSENT ((size_t)-1)   /* the offset of a region the solver does not have */

typedef struct {
  int m, T, ts;           /* local rows, enlarging factor, panel stride */
  int ortho_alg;
  int spmm_cap, bj_cap;   /* Gram blocks the SpMM / the block solve can leave behind, 0: none */
  int G, S;               /* pa_gram_max_blocks(), pa_finish32_scratch_blocks() */
} pa_ecg_pool_in_t;

/* Offsets in doubles from the start of the pool, in the order of the regions. */
typedef struct {
  size_t v[2], av[2];     /* P / P_prev and AP / AP_prev slots; [1] absent for Orthomin */
  size_t z, r, x;
  size_t F;               /* [alpha T^2 | beta 2T^2 | mu T^2 | rtr T^2] */
  size_t alpha, beta, mu, rtr;
  size_t q;               /* 2T^2 */
  size_t res2;            /* 24: the pair + 16 sums */
  size_t uu;              /* 2T^2 */
  size_t partials;        /* G * 2 ts^2 */
  size_t rtr_part;        /* G * ts */
  size_t spmm_parts;      /* (spmm_cap + S) * 32, absent at capacity 0 */
  size_t bj_parts;        /* (bj_cap + S) * 32, absent at capacity 0 */
  size_t grp;             /* 48: the per-system sums of several right-hand sides (and the caller's ||b_j||^2 of a system solve) */
  size_t sys_part;        /* G * ts: the partial sums of pa_k_sys_gather / pa_k_sys_norms */
  size_t pool_doubles;    /* the end of sys_part */
} pa_ecg_pool_t;
void pa_ecg_pool_layout(const pa_ecg_pool_in_t* in, pa_ecg_pool_t* out);

typedef struct {
  int ortho_alg, bs_red, enlFac;
  int nrhs, guess, metric;        /* the systems the solver will hold; a start from a guess; the caller's stopping metric */
  int world, loopback, timing;    /* pa_world_size(), pa_comm_is_loopback(), pa_timing_enabled() */
  /* the switches as the caller read them */
  int fuse, lazy_norm, lazy_stop;
  int graphs;                     /* the graph request: 0, 1, or 2 = for any process group */
  int poll;                       /* -1: unset, else 0 / 1 */
} pa_ecg_switch_in_t;
/* ride: several systems on several processes; ride_sys: the caller's metric on several processes (whatever nrhs):
 * in both the per-system sums of the stopping test travel behind the pair [norm^2, status] of a collective the
 * iteration has anyway (ecg.c: pa_ecg_queue_group_norms).  ride_sys stands last: the fields before it keep their place. */
typedef struct { int rotate, fuse, lazy_norm, lazy_stop, use_graphs, poll, ride, ride_sys; } pa_ecg_switch_t;
void pa_ecg_switches(const pa_ecg_switch_in_t* in, pa_ecg_switch_t* out);

int pa_ecg_solve_first_rule(int on, int nprocs, int ortho_alg, int bs_red, int enlFac, int fuse, int lazy_norm,
                            int lazy_stop, int bj_gram, int spmm_gram, int graphs);

/* What a row pass of solve_first_step does with X (the values are the kernel's: pa_k_update_xrz_mode).  on: the
 * switch PREALPS_ECG_X_DEFER; pending: the pass before this one left its update of X owed; another_step_follows: this
 * call of the library's loop queues another row pass behind this one unless the iteration stops.
 *   pending                    -> BOTH: the owed update and this one (the caller clears pending);
 *   on, another step follows   -> SKIP: X stays where it is (the caller sets pending);
 *   otherwise                  -> EVERY.
 * So no two passes in a row skip, a pass that may be the call's last owes nothing, and a debt is left only by a stop
 * (which pa_k_flush_x pays before anything else can look at X). */
enum { PA_ECG_X_EVERY = 0, PA_ECG_X_SKIP = 1, PA_ECG_X_BOTH = 2 };
int pa_ecg_x_mode(int on, int pending, int another_step_follows);

#endif
