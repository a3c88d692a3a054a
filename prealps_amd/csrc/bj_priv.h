/*
 * bj_priv.h -- what the three units of the block-Jacobi preconditioner share: block_jacobi.c (state, create,
 * apply), bj_update.c (preAlps_BlockJacobiUpdateValues) and bj_coarse.c (the coarse space).  The host work of the
 * create and the layout table are bj_build.h's, pure host code; everything here may touch the device.
 */
#ifndef PA_BJ_PRIV_H
#define PA_BJ_PRIV_H

#include "pa_host.h"
#include "bj_build.h"
#include "bj_share.h"
#include "coarse_space.h"

/* The coarse space attached to the preconditioner (preAlps_BlockJacobiSetCoarseSpace): what the caller gave, kept on
 * the host for preAlps_BlockJacobiUpdateValues, and the device arrays pa_k_coarse_apply reads. */
typedef struct {
  int on;
  int k, naggr, nc, nchunks, n;
  int nparts;                 /* entries of part_aggregate */
  double* V;                  /* the caller's vectors, n x k column major, in the caller's order and units */
  int* part_aggregate;        /* the operator's nparts: the parts of all processes */
  int multi;                  /* attached on several processes: d_Einv holds the nrows rows of the inverse listed in d_rows */
  int nrows; int* d_rows;
  double* d_zv; int* d_ch_row0; int* d_ch_nrows; int* d_ch_aggr; int* d_agg_ptr; int* d_agg_chunk;
  double* d_Einv; double* d_partial; double* d_c; double* d_y;
  pa_coarse_plan_t plan;
  double bytes, setup_s;
  int builds; long long applies;
} pa_bj_coarse_t;

typedef struct {
  int created;
  pa_bj_coarse_t co;
  int np;                 /* local blocks */
  int m;
  /* device */
  int* d_row0; int* d_nrows; int* d_bw; long long* d_off;
  int* d_map_f; int* d_map_b;
  double* d_Lf; double* d_Lb; double* d_invd_f; double* d_invd_b;
  double* d_Lf2; double* d_Lb2; long long* d_off2;     /* paired records of the narrow classes (optional) */
  double pairs_bytes;
  /* Where the apply READS a block's records (bj_share.h): off_read[p] = off[rep[p]], off2_read[p] = off2[rep[p]].
   * Every block keeps its own slot at off / off2 and every set-up kernel keeps writing it; the plan gets these two.
   * A refresh turns a block whose band no longer equals its representative's back to its own slot
   * (bj_refactor.hip: k_bj_share_check); the pointers never change, so captured graphs stay valid. */
  long long* d_off_read; long long* d_off2_read;
  int* d_rep; int* d_share_list; unsigned long long* d_share_cnt;   /* rep, the blocks with rep[p] != p, the check's two sums */
  int share_on, share_classes, share_members, shared_blocks;       /* members: blocks with rep[p] != p at the create */
  long long shared_elems2;                                         /* second-record elements of the blocks that share now */
  double share_s;                                                  /* seconds of the class pass */
  /* The pair tasks of the classes that bj_g4.hip serves from fp64 records (bj_share.h: pa_bj_pair_tasks), built at the
   * create from the create's classes and never changed: the PAIR launch is only taken while no class has split
   * (plan.pair_intact, set again by every refresh; the rule itself is the launch planner's, bj_g4_plan.c). */
  int* d_ptask[PA_BJ_MAX_CLASSES]; pa_bj_ptask_t class_ptask[PA_BJ_MAX_CLASSES];
  int pair_mode, pair_tasks, paired_blocks;                        /* PREALPS_BJ_PAIR as the create read it; sums over the classes */
  void* d_Lg4; int g4_bits; double g4_bytes;                   /* one-copy records of bj_g4.hip (optional) */
  int* d_class_list[PA_BJ_MAX_CLASSES];                        /* the block list of every class of the layout */
  const int* class_list_c[PA_BJ_MAX_CLASSES];
  pa_bj_plan_t plan;
  double factor_bytes; int nd_blocks;
  /* The layout of the create (bj_build.h), kept until the preconditioner is freed: the plan's class table points
   * into it, and preAlps_BlockJacobiUpdateValues launches on its offsets and lists, so that it repeats no decision. */
  pa_bj_layout_t lay;
  /* What else preAlps_BlockJacobiUpdateValues needs of the create, so that it reads no switch again: the host
   * copies of the per-block arrays and of the factor order, the switches as the create read them, and what tells
   * that operator and panel are still the create's. */
  int* h_row0; int* h_nrows; int* h_bw; int* h_grow0; int* h_map_f; char* h_is_nd;
  int* h_rep;                    /* np: the block whose records a block read at the create (bj_share.h), never changed */
  int row_off, dev_factor, dev_wmax, nd_bits;
  const int* A_rowptr;           /* rowPtr of the create's A */
  int op_build;                  /* pa_operator_build_count() at the create */
  /* the band map on the device (bj_band_map.h) and the device copies of the layout's band offsets and launch
   * lists, cut at the first update and kept until the preconditioner is freed */
  unsigned* d_bm_src; unsigned* d_bm_dst; int* d_bm_chunk_blk; unsigned* d_bm_chunk_first;
  size_t bm_n, bm_nchunks, bm_bytes;
  long long* d_boff; int* d_slist; int* d_blist; int* d_fail;
  int bm_builds, updates, nd_rebuilt;
  double upd_map_s, upd_copy_s, upd_kernel_s, upd_total_s;
} pa_bj_t;

/* ---- block_jacobi.c ---------------------------------------------------------------------------------------- */
pa_bj_t* pa_bj_state(void);             /* the one instance */
void pa_bj_apply_epoch_bump(void);      /* pa_bj_apply_epoch() + 1 */
void pa_bj_values_epoch_sync(void);     /* pa_bj_values_epoch() = the operator's, after a create or a refresh */
/* The two factorisation kernels on the layout's lists (d_slist / d_blist / d_boff their device copies) and
 * the records of s, then *fail = 1 + local position of a non-positive pivot (0: none) read back from d_fail,
 * which the caller zeroed.  Non-zero: a launch or the copy failed (pa_rt_error()). */
int pa_bj_factor_launch(const pa_bj_t* s, const int* d_slist, const int* d_blist, const long long* d_boff,
                        double* d_band, int* d_fail, int* fail);
/* the global row of that pivot */
int pa_bj_fail_global_row(int row_off, const int* map_f, const int* row0, const int* nrows, int np, int fail);
/* The sparse-factored blocks (the nnd flagged in is_nd) go to nd.c; a failure is reported as `who`. */
int pa_bj_nd_handoff(const char* who, const CPLM_Mat_CSR_t* A, int np, const char* is_nd, int nnd, const int* row0,
                     const int* nrows, const int* grow0, int m, int bits, int row_off);
/* The launches that fill the second layouts from the plain records (the create, and the refactorisation in place). */
int pa_bj_launch_g4(const pa_bj_t* s);
int pa_bj_launch_pairs(const pa_bj_t* s);

/* ---- bj_coarse.c ------------------------------------------------------------------------------------------ */
void pa_bj_coarse_release(pa_bj_coarse_t* co);
/* after new values: zv, E and Einv again into the same device arrays; a failure drops the coarse space.  Collective on
 * several processes, where the failure of one drops it on all. */
int pa_bj_coarse_refresh(pa_bj_t* s, const pa_operator_info_t* op);

#endif
