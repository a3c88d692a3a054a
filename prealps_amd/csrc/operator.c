/*
 * operator.c -- the global-static linear operator of the ECG drivers, resident
 * in HBM.  Host side of the SpMM hot path.
 *
 * Reference behaviour kept (all under /root/reference):
 *   preAlps_OperatorBuild      utils/operator.c:38-134    load -> scale ->
 *                              partition -> permute -> row panels
 *   MatrixMarket reader        mtx_read.c
 *   scaling, ordering, panel   op_build.c (the shard of this process on the host; adopt_shard takes it over)
 *   preAlps_BlockOperator      utils/operator.c:334-351 ->
 *                              utils/cplm_v0/cplm_v0_matmult_v2.c:108-343
 *   getters                    utils/operator.c:353-393
 *
 * MI355X design instead of the reference's: the number of subdomains is
 * `nparts` (not the process count); a process owns a contiguous range of
 * parts; only boundary rows travel between processes (the reference ships
 * whole panels); the O(m*P) colPos table is replaced by row blocks with an
 * interior / halo-reading split so the exchange overlaps the interior SpMM.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pa_host.h"
#include "mtx_read.h"
#include "op_build.h"
#include "pa_alloc.h"
#include "spmm_plan.h"
#include "spmm_code.h"
#include "spmm_pack.h"

typedef struct {
  pa_operator_info_t info;
  int lnnz;
  /* SpMM plan: SELL-64 slices with local column ids + workgroup blocks (spmm_plan.h) */
  pa_spmm_plan_t plan;
  void* d_plan[PA_PL_COUNT];   /* the device arrays `plan` points into */
  double sell_entries;   /* stored entries including padding */
  int* lcol;             /* host: local column ids of the panel (own rows < m <= halo slots) */
  int plan_ts;           /* panel stride the current SpMM plan was cut for (0: none) */
  double stream_bytes;   /* bytes of matrix data one SpMM streams */
  /* halo exchange */
  int npeers;
  int* peers;        /* process ids */
  int* send_rows;    /* per peer, rows */
  int* recv_rows;
  int* send_cnt;     /* scratch: elements for the current stride */
  int* recv_cnt;
  int nsend;         /* total rows packed */
  int* send_idx;     /* local rows packed for the peers, peer after peer */
  int* halo_cols;    /* global row of every halo slot, ascending */
  int* d_send_idx;
  int* d_pk_off; int* d_pk_slot;   /* the inverse of send_idx: row r is packed into slots pk_slot[pk_off[r] .. pk_off[r + 1]) */
  const double* prepacked;         /* the panel whose send rows the solver's update kernel has already packed (pa_operator_pack_hint) */
  double* d_sendbuf; double* d_halo;
  int buf_ts;        /* stride the buffers are sized for */
  void* ev_packed;   /* send buffer is packed (main stream) */
  void* ev_halo;     /* halo rows have arrived (side stream) */
  int* colPos_dummy;
  /* an update of the values in place (preAlps_OperatorUpdateValues); nothing else reads these */
  int from_csr;        /* built by preAlps_OperatorBuildFromCSR for the caller: the value order is the caller's */
  int scaled;
  int* src_rowptr;     /* the caller's rowPtr (N + 1): the rows of the scaling vector */
  int* src;            /* panel entry -> index into the caller's val (lnnz) */
  int plan_staged_sw, plan_runs_sw, plan_cus;   /* what build_plan gave the builders for the current plan */
  size_t plan_val_n;   /* values of the host plan's value array (packed or not: what the value map counts) */
  /* the packed value array of a run plan (spmm_pack.h): plan.val holds pk_nval values and the slack, plan.pk_meta
   * the masks and offsets; the unpacked array is then not on the device */
  size_t pk_nval;
  double pk_stream_bytes;   /* bytes of matrix data one product streams from the packed plan */
  int repacks;              /* updates of the values that had to pack anew */
  /* the fp32 copy of the packed array (preAlps_hip_set_operator_precision(32)): pk_nalloc floats -- every element of
   * plan.val, the steps' zeros and the slack included -- at plan.val32; plan.val stays where it is */
  size_t pk_nalloc;         /* elements of the packed array as allocated */
  int plan_pack_sw;         /* PREALPS_SPMM_PACK as the current plan was cut under */
  int val32_owed;           /* the copy was refused after new values while 32 stays in force: the next product forms it or fails */
  /* the 2-byte codes of the packed array and their per-block tables (spmm_code.h), beside plan.val, which stays */
  int plan_code_sw;         /* PREALPS_SPMM_CODE as the current plan was cut under (-1: the rule decides) */
  int code_blocks;          /* coded blocks */
  size_t code_entries;      /* table entries of all blocks */
  double code_stream_bytes; /* bytes of matrix data one product streams from the coded plan */
  int recodes;              /* updates of the values that formed the codes anew */
  unsigned* d_vmap;    /* device: stored value -> panel entry + 1, 0 = padding (plan_val_n entries; NULL: not cut yet) */
  int values_epoch;    /* 0 after a build, + 1 per update */
  int vmap_builds;     /* value maps cut for this operator */
  /* the row map of preAlps_ECGSolveSystem on the device, cut at the first system solve: for local row i the caller's
   * row src[i] = perm[row_off + i] and its scaling factor dl[i] = d[src[i]] (1.0 when unscaled), 12 bytes per row */
  int* d_sys_src; double* d_sys_dl;
  int sys_map_epoch;   /* values_epoch when it was cut: an update of the values moves d */
  int sys_map_builds;
} pa_operator_t;

static pa_operator_t g_op;
/* + 1 per change of what a product launches or reads (pa_operator_plan_epoch); never reset, so that a solver kept across
 * a free and a rebuild of the operator cannot meet the count it last saw */
static int g_plan_epoch;
static int g_op_builds;   /* operators built so far (pa_operator_build_count) */
static double g_setup_build_s, g_setup_plan_s;   /* host seconds: scale/permute/halo lists, SpMM plan */

const pa_operator_info_t* pa_operator_info(void) { return g_op.info.built ? &g_op.info : NULL; }

/* ------------------------------------------------------------------ utils */
static size_t g_dbg_val_bytes, g_dbg_slot_bytes;   /* device bytes of the run plan's values / slots */

static int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

/* --------------------------------------------------------------- free ---- */
static void free_codes(pa_operator_t* o) {
  pa_rt_free((void*)o->plan.code); pa_rt_free((void*)o->plan.code_tab); pa_rt_free((void*)o->plan.blk_tab_off);
  o->plan.code = NULL; o->plan.code_tab = NULL; o->plan.blk_tab_off = NULL;
  o->plan.coded = 0; o->plan.code_lds = 0;
  o->code_blocks = 0; o->code_entries = 0; o->code_stream_bytes = 0.0;
}

static void free_plan(pa_operator_t* o) {
  for (int i = 0; i < PA_PL_COUNT; ++i) { pa_rt_free(o->d_plan[i]); o->d_plan[i] = NULL; }
  o->plan_ts = 0;
  pa_rt_free((void*)o->plan.pk_meta);
  pa_rt_free((void*)o->plan.val32);
  free_codes(o);
  memset(&o->plan, 0, sizeof(o->plan));
  o->pk_nalloc = 0; o->val32_owed = 0;
  ++g_plan_epoch;
  pa_rt_free(o->d_vmap); o->d_vmap = NULL;   /* the value map belongs to the plan */
  o->plan_val_n = 0;
  o->pk_nval = 0; o->pk_stream_bytes = 0.0;
}

void preAlps_OperatorFree(void) {
  pa_operator_t* o = &g_op;
  preAlps_SolutionHistoryFree();      /* (the history belongs to the operator) */
  free_plan(o);
  free(o->lcol); free(o->src); free(o->src_rowptr);
  free(o->info.rowPos); free(o->info.perm); free(o->info.scaling);
  pa_rt_free(o->d_sys_src); pa_rt_free(o->d_sys_dl);
  free(o->info.A.rowPtr); free(o->info.A.colInd); free(o->info.A.val);
  free(o->peers); free(o->send_rows); free(o->recv_rows); free(o->send_cnt); free(o->recv_cnt);
  free(o->send_idx); free(o->halo_cols);
  pa_rt_event_destroy(o->ev_packed); pa_rt_event_destroy(o->ev_halo);
  pa_rt_free(o->d_send_idx); pa_rt_free(o->d_sendbuf); pa_rt_free(o->d_halo);
  pa_rt_free(o->d_pk_off); pa_rt_free(o->d_pk_slot);
  free(o->colPos_dummy);
  memset(o, 0, sizeof(*o));
}

/* ------------------------------------------------------------ the plan ---- */
/* The packed value array and its masks into fresh device arrays (pk may be released afterwards). */
static int upload_pack(const pa_spmm_pack_t* pk, void** d_val, void** d_meta) {
  *d_val = pa_rt_malloc(pk->nval_alloc * sizeof(double));
  *d_meta = pa_rt_malloc(pk->nsteps_alloc * 4 * sizeof(uint64_t));
  if (!*d_val || !*d_meta || pa_rt_h2d(*d_val, pk->val, pk->nval_alloc * sizeof(double)) ||
      pa_rt_h2d(*d_meta, pk->meta, pk->nsteps_alloc * 4 * sizeof(uint64_t))) {
    pa_rt_free(*d_val); pa_rt_free(*d_meta);
    *d_val = *d_meta = NULL;
    return 1;
  }
  return 0;
}

/* The plan is cut on the host (spmm_plan.c); here it goes to the device: every array of the host
 * plan into a device array of its own, owned by o->d_plan[], and the pointers into o->plan.
 * pk != NULL: the values go up packed (spmm_pack.h) and the host plan's own value array stays on the host. */
static int upload_plan(pa_operator_t* o, const pa_spmm_host_plan_t* hp, const pa_spmm_pack_t* pk) {
  for (int i = 0; i < PA_PL_COUNT; ++i) {
    const pa_plan_array_t* a = &hp->a[i];
    if (!a->p || (pk && i == PA_PL_VAL)) continue;
    o->d_plan[i] = pa_rt_malloc(a->n_alloc * a->elem);
    if (!o->d_plan[i] || pa_rt_h2d(o->d_plan[i], a->p, a->n * a->elem)) return 1;
  }
  pa_spmm_plan_t* pl = &o->plan;
  if (pk) {
    void* d_meta = NULL;
    if (upload_pack(pk, &o->d_plan[PA_PL_VAL], &d_meta)) return 1;
    pl->packed = 1; pl->pk_meta = (const unsigned long long*)d_meta;
    o->pk_nval = pk->nval; o->pk_nalloc = pk->nval_alloc;
    o->pk_stream_bytes = hp->stream_bytes - pk->unpacked_bytes + pk->packed_bytes;
  }
  pl->m = hp->m; pl->nslices = hp->nslices; pl->nblk = hp->nblk; pl->n_interior = hp->n_interior;
  pl->win_cap = hp->win_cap; pl->staged = hp->staged; pl->stage_cap = hp->stage_cap;
  pl->runs = hp->runs; pl->runs_cols = hp->runs_cols;
  pl->sl_off = o->d_plan[PA_PL_SL_OFF]; pl->sl_len = o->d_plan[PA_PL_SL_LEN];
  pl->sl_row0 = o->d_plan[PA_PL_SL_ROW0]; pl->sl_nrows = o->d_plan[PA_PL_SL_NROWS];
  pl->col = o->d_plan[PA_PL_COL]; pl->col16 = o->d_plan[PA_PL_COL16]; pl->val = o->d_plan[PA_PL_VAL];
  pl->blk_slice = o->d_plan[PA_PL_BLK_SLICE]; pl->blk_win = o->d_plan[PA_PL_BLK_WIN];
  pl->blk_ext_off = o->d_plan[PA_PL_BLK_EXT_OFF]; pl->blk_nlow = o->d_plan[PA_PL_BLK_NLOW];
  pl->ext_rows = o->d_plan[PA_PL_EXT_ROWS]; pl->order = o->d_plan[PA_PL_ORDER];
  o->sell_entries = hp->sell_entries;
  o->stream_bytes = hp->stream_bytes;
  o->plan_val_n = hp->a[PA_PL_VAL].n;
  if (hp->runs) {   /* what preAlps_hip_debug_move_plan copies */
    g_dbg_val_bytes = pk ? pk->nval_alloc * sizeof(double) : hp->a[PA_PL_VAL].n_alloc * hp->a[PA_PL_VAL].elem;
    g_dbg_slot_bytes = hp->a[PA_PL_COL16].n_alloc * hp->a[PA_PL_COL16].elem;
  }
  return 0;
}

/* ---- the packed values as 2-byte codes (spmm_code.h) ----
 * A packed run plan at 2 or 4 columns with fp64 storage is coded when that takes a tenth off what the packed plan
 * streams: matrices assembled from one element matrix (Q1 elasticity: a few dozen distinct values per block).
 * PREALPS_SPMM_CODE=0 never codes, =1 codes every block that fits whatever it saves.  The codes go into device arrays
 * of their own; the old ones go only when the new ones are up.  A plan the rule leaves alone holds no codes. */
static int code_plan(pa_operator_t* o, const pa_spmm_host_plan_t* hp, const pa_spmm_pack_t* pk, int ts, int bits) {
  const int sw = o->plan_code_sw;
  if (sw == 0 || bits != 64 || (ts != 2 && ts != 4) || !hp->runs || hp->runs_cols != ts) {
    if (o->plan.coded) { free_codes(o); ++g_plan_epoch; }
    return 0;
  }
  pa_spmm_code_t cd;
  int crc = pa_spmm_code_build(pk, (const int*)hp->a[PA_PL_BLK_SLICE].p, hp->nblk, (const long long*)hp->a[PA_PL_SL_OFF].p,
                               (const int*)hp->a[PA_PL_SL_ROW0].p, (const int*)hp->a[PA_PL_SL_NROWS].p,
                               (const int*)hp->a[PA_PL_BLK_EXT_OFF].p, hp->runs, ts, 32768, &cd);
  if (crc == -1) return PA_FAIL("out of host memory for the codes of the SpMM plan");
  const double packed_stream = hp->stream_bytes - pk->unpacked_bytes + pk->packed_bytes;
  const double coded_stream = hp->stream_bytes - pk->unpacked_bytes + cd.coded_bytes;
  const int code = crc == 0 && cd.ncoded > 0 && (sw > 0 || coded_stream < 0.9 * packed_stream);
  if (!code) {
    pa_spmm_code_free(&cd);
    if (o->plan.coded) { free_codes(o); ++g_plan_epoch; }
    return 0;
  }
  void* d_code = pa_rt_malloc(cd.ncode * sizeof(uint16_t));
  void* d_tab = pa_rt_malloc((cd.ntab ? cd.ntab : 1) * sizeof(double));
  void* d_off = pa_rt_malloc(((size_t)cd.nblk + 1) * sizeof(int));
  if (!d_code || !d_tab || !d_off || pa_rt_h2d(d_code, cd.code, cd.ncode * sizeof(uint16_t)) ||
      pa_rt_h2d(d_tab, cd.tab, cd.ntab * sizeof(double)) || pa_rt_h2d(d_off, cd.blk_tab_off, ((size_t)cd.nblk + 1) * sizeof(int))) {
    pa_rt_free(d_code); pa_rt_free(d_tab); pa_rt_free(d_off);
    pa_spmm_code_free(&cd);
    return PA_FAIL("uploading the codes of the SpMM plan failed: %s", pa_rt_error());
  }
  free_codes(o);
  o->plan.code = (const unsigned short*)d_code; o->plan.code_tab = (const double*)d_tab; o->plan.blk_tab_off = (const int*)d_off;
  o->plan.code_lds = cd.lds_bytes; o->plan.coded = 1;
  o->code_blocks = cd.ncoded; o->code_entries = cd.ntab; o->code_stream_bytes = coded_stream;
  ++g_plan_epoch;
  pa_spmm_code_free(&cd);
  return 0;
}

/* What the builders are given for stride ts: the panel and the switches of the current plan. */
static pa_spmm_plan_in_t plan_input(const pa_operator_t* o, int ts) {
  const pa_operator_info_t* in = &o->info;
  pa_spmm_plan_in_t pin = {
    .m = in->m, .halo = in->halo, .part0 = in->part0, .part1 = in->part1, .row_off = in->row_off,
    .rowPos = in->rowPos, .rowPtr = in->A.rowPtr, .lcol = o->lcol, .val = in->A.val,
    .ts = ts, .cus = o->plan_cus, .want_staged = o->plan_staged_sw, .want_runs = o->plan_runs_sw};
  return pin;
}

/* ---- storage of the matrix values (preAlps_hip_set_operator_precision) ----
 * 64 / 32 bits; 0 = follow PREALPS_SPMM_PRECISION (double, the default, or single).  fp32 reaches the packed run plan
 * at a panel stride of at most 4 columns and nothing else: every other plan keeps its fp64 values and its bits. */
static int g_op_bits = 0;
static double g_round_kernel_s;      /* device seconds of the last k_plan_round_values */
/* the storage in force: 64 or 32; -1 (reported): the variable holds something else */
static int operator_bits(void) {
  if (g_op_bits) return g_op_bits;
  const char* pe = getenv("PREALPS_SPMM_PRECISION");
  if (!pe || !*pe || !strcmp(pe, "double")) return 64;
  if (!strcmp(pe, "single")) return 32;
  PA_FAIL("PREALPS_SPMM_PRECISION=%s: expected double or single (storage of the matrix values of the SpMM)", pe);
  return -1;
}
static void drop_val32(pa_operator_t* o) {
  if (!o->plan.val32) return;
  pa_rt_free((void*)o->plan.val32);
  o->plan.val32 = NULL;
  ++g_plan_epoch;
}
/* The fp32 copy of the packed array as it stands (k_plan_round_values), into the allocation that is there or a new
 * one of pk_nalloc floats.  A value that fp32 cannot hold frees the copy and is reported. */
static int form_val32(pa_operator_t* o) {
  float* d32 = (float*)o->plan.val32;
  const int fresh = d32 == NULL;
  unsigned long long bad[2] = {0, 0};
  unsigned long long* d_bad = (unsigned long long*)pa_rt_malloc(sizeof(bad));
  if (fresh) d32 = (float*)pa_rt_malloc((o->pk_nalloc ? o->pk_nalloc : 1) * sizeof(float));
  void* e0 = pa_rt_event_create();
  void* e1 = pa_rt_event_create();
  int rc = !d_bad || !d32 || !e0 || !e1 || pa_rt_memset(d_bad, 0, sizeof(bad)) || pa_rt_event_record(e0) ||
           pa_k_plan_round_values(o->plan.val, d32, o->pk_nalloc, d_bad) || pa_rt_event_record(e1) ||
           pa_rt_d2h(bad, d_bad, sizeof(bad)) || pa_rt_sync();
  if (!rc) g_round_kernel_s = pa_rt_event_elapsed_s(e0, e1);
  pa_rt_event_destroy(e0); pa_rt_event_destroy(e1);
  pa_rt_free(d_bad);
  if (rc || bad[0]) {
    pa_rt_free(d32);
    o->plan.val32 = NULL;
    o->val32_owed = 1;
    ++g_plan_epoch;
    if (rc) return PA_FAIL("the single-precision copy of the matrix values: %s", pa_rt_error());
    double v;
    memcpy(&v, &bad[1], sizeof(v));
    return PA_FAIL("single precision cannot hold %llu of the matrix values (one of them: %.17g); the operator keeps "
                   "double (scale the operator, or preAlps_hip_set_operator_precision(64))", bad[0], v);
  }
  if (fresh) { o->plan.val32 = d32; ++g_plan_epoch; }
  o->val32_owed = 0;
  return 0;
}

/* The switches are read at every build: tests and probes change them between builds in one process. */
static int build_plan(pa_operator_t* o, int ts) {
  const int bits = operator_bits();
  if (bits < 0) return 1;
  free_plan(o);
  o->plan_cus = pa_rt_num_cus();
  o->plan_staged_sw = env_int("PREALPS_SPMM_STAGED", -1);
  o->plan_runs_sw = env_int("PREALPS_SPMM_RUNS", 1);
  pa_spmm_plan_in_t pin = plan_input(o, ts);
  pa_spmm_host_plan_t hp;
  if (pa_spmm_plan_build(&pin, &hp))
    return hp.oom_entries ? PA_FAIL("out of host memory for %zu SELL entries", hp.oom_entries)
                          : PA_FAIL("out of host memory for the SpMM plan");
  /* A run plan at up to 4 columns goes up without its stored +0.0 values (spmm_pack.h) when that takes a tenth
   * off the matrix stream: whole element matrices assembled into the pattern (Q1 elasticity: 37 % zeros) and the
   * padding.  PREALPS_SPMM_PACK=0 / 1 forces. */
  pa_spmm_pack_t pk;
  int packed = 0;
  const int pack_sw = env_int("PREALPS_SPMM_PACK", -1);
  o->plan_pack_sw = pack_sw;
  /* (fp32 storage lives behind the masks of the pack: with 32 in force such a plan is packed whatever it saves) */
  if (hp.runs && hp.runs_cols == ts && ts <= 4 && pack_sw != 0) {
    int prc = pa_spmm_pack_build((const double*)hp.a[PA_PL_VAL].p, (const long long*)hp.a[PA_PL_SL_OFF].p,
                                 (const int*)hp.a[PA_PL_SL_LEN].p, hp.nslices, 0, &pk);
    if (prc == -1) { pa_spmm_plan_free(&hp); return PA_FAIL("out of host memory for the packed values of the SpMM plan"); }
    packed = prc == 0 && (pack_sw > 0 || bits == 32 || hp.stream_bytes - pk.unpacked_bytes + pk.packed_bytes < 0.9 * hp.stream_bytes);
    if (prc == 0 && !packed) pa_spmm_pack_free(&pk);
  }
  o->plan_code_sw = env_int("PREALPS_SPMM_CODE", -1);
  int rc = upload_plan(o, &hp, packed ? &pk : NULL);
  if (rc) PA_FAIL("uploading the SpMM plan failed: %s", pa_rt_error());
  else if (packed) rc = code_plan(o, &hp, &pk, ts, bits);
  if (packed) pa_spmm_pack_free(&pk);
  pa_spmm_plan_free(&hp);
  if (rc) { free_plan(o); return 1; }
  o->plan_ts = ts;
  if (packed && bits == 32 && form_val32(o)) { free_plan(o); return 1; }
  return 0;
}


/* -------------------------------------------------------------- build ---- */
static int g_plan_only = 0;
/* Host-side planning without touching the GPU (sharding, halo lists): what the
 * multi-process CPU tests exercise.  BlockOperator is unavailable in this mode. */
void preAlps_hip_plan_only(int on) { g_plan_only = on ? 1 : 0; }
int pa_operator_plan_only(void) { return g_plan_only; }

/* ---- the build, in three steps (op_build.c: the shard on the host) --------------------------
 * (1) pa_op_order: what needs the whole matrix -- the diagonal check, the scaling vector of
 *     SymRACScaling and the ordering that groups rows part by part (rank 0 only when the set-up is
 *     distributed);
 * (2) pa_op_panel: this process's row panel from its raw rows (scaled, renumbered, sorted), the
 *     halo slots and who owns them;
 * (3) the send lists: from the whole matrix when every process holds it (pa_op_peers_whole), else by
 *     asking the owners (pa_mpi_swap_lists, pa_op_finish_peers);
 * then adopt_shard: the upload, and the finished shard into g_op. */
static int setup_trace(void) { return getenv("PREALPS_SETUP_TRACE") != NULL; }
#define TRACE_DECL double t_tr = pa_wtime(); const int tr = setup_trace()
#define TRACE(what) do { if (tr) { double n_ = pa_wtime(); fprintf(stderr, "[setup] %-28s %.3f s\n", what, n_ - t_tr); t_tr = n_; } } while (0)

/* The one place where a shard becomes the operator: whatever can fail comes first (the scratch of the
 * exchange, the send list on the device), then the pointers move and *sh is left empty.  A failure leaves
 * g_op as preAlps_OperatorFree leaves it and *sh to the caller.  src_rowptr (taken over on success): the
 * caller's rowPtr when the values keep the caller's order, else NULL. */
static int adopt_shard(pa_operator_t* o, pa_op_shard_t* sh, int size, long long nnz_global, int* src_rowptr, int scaled,
                       double t_build0) {
  const size_t room = (size_t)(size > 0 ? size : 1);
  int* send_cnt = (int*)calloc(room, sizeof(int));
  int* recv_cnt = (int*)calloc(room, sizeof(int));
  int* d_send_idx = NULL;
  if (!send_cnt || !recv_cnt) { free(send_cnt); free(recv_cnt); return PA_FAIL("out of host memory"); }
  if (!g_plan_only && sh->nsend > 0) {
    d_send_idx = (int*)pa_rt_malloc((size_t)sh->nsend * sizeof(int));
    if (!d_send_idx || pa_rt_h2d(d_send_idx, sh->send_idx, (size_t)sh->nsend * sizeof(int))) {
      pa_rt_free(d_send_idx); free(send_cnt); free(recv_cnt);
      return PA_FAIL("uploading the operator failed: %s", pa_rt_error());
    }
  }
  pa_operator_info_t* in = &o->info;
  in->N = sh->N; in->nparts = sh->nparts; in->part0 = sh->part0; in->part1 = sh->part1;
  in->rank = pa_world_rank(); in->world = size; in->loopback = pa_comm_is_loopback();
  in->row_off = sh->row_off; in->m = sh->m; in->halo = sh->halo;
  in->rowPos = sh->rowPos; in->perm = sh->perm;
  in->scaling = sh->d;     /* (kept: preAlps_OperatorGetScalingPtr, the row map of preAlps_ECGSolveSystem) */
  CPLM_Mat_CSR_t* A = &in->A;
  A->rowPtr = sh->rowPtr; A->colInd = sh->colInd; A->val = sh->val;
  A->info.M = sh->N; A->info.N = sh->N; A->info.nnz = (int)(nnz_global > 2147483647LL ? 2147483647LL : nnz_global);
  A->info.m = sh->m; A->info.n = sh->N;
  A->info.lnnz = sh->lnnz; A->info.blockSize = 1; A->info.format = FORMAT_CSR;
  A->info.structure = UNSYMMETRIC;
  o->lnnz = sh->lnnz; o->lcol = sh->lcol; o->src = sh->src; o->halo_cols = sh->halo_cols;
  o->npeers = sh->npeers; o->nsend = sh->nsend;
  o->peers = sh->peers; o->send_rows = sh->send_rows; o->recv_rows = sh->recv_rows; o->send_idx = sh->send_idx;
  o->send_cnt = send_cnt; o->recv_cnt = recv_cnt; o->d_send_idx = d_send_idx;
  if (src_rowptr) { o->src_rowptr = src_rowptr; o->from_csr = 1; o->scaled = scaled; }
  free(sh->iperm); free(sh->recv_by_proc);
  memset(sh, 0, sizeof(*sh));
  ++g_op_builds;
  in->built = 1;
  if (!g_plan_only) g_setup_build_s = pa_wtime() - t_build0;
  return 0;
}

/* keep_src: the values keep the caller's order (preAlps_OperatorUpdateValues may follow); 0 when the matrix came
 * from a file, whose value order is not the caller's. */
static int build_from_csr(int N, const int* rowPtr, const int* colInd, const double* val, int nparts, const int* part,
                          int scale, int keep_src) {
  if (!g_plan_only) PA_REQUIRE_GPU();
  if (g_op.info.built) preAlps_OperatorFree();
  double t_build0 = pa_wtime();
  const int size = pa_world_size();
  if (N < 1 || nparts < 1 || nparts > N) return PA_FAIL("invalid sizes N=%d nparts=%d", N, nparts);
  if (nparts < size)
    return PA_FAIL("Each process needs at least one block (nparts = %d < %d = processes)", nparts, size);
  const pa_op_in_t bin = {.N = N, .rowPtr = rowPtr, .colInd = colInd, .val = val, .nparts = nparts, .part = part,
                          .scale = scale, .rank = pa_world_rank(), .size = size, .threads = pa_host_threads(),
                          .trace = setup_trace()};
  pa_op_shard_t sh;
  char err[256];
  if (pa_op_order(&bin, &sh, err, sizeof(err)) || pa_op_panel(&bin, &sh, 1, keep_src, err, sizeof(err)) ||
      pa_op_peers_whole(&bin, &sh, err, sizeof(err)))
    return PA_FAIL("%s", err);
  int* src_rowptr = NULL;
  if (keep_src) {
    src_rowptr = (int*)malloc(((size_t)N + 1) * sizeof(int));
    if (!src_rowptr) { pa_op_shard_free(&sh); return PA_FAIL("out of host memory"); }
    memcpy(src_rowptr, rowPtr, ((size_t)N + 1) * sizeof(int));
  }
  if (adopt_shard(&g_op, &sh, size, (long long)rowPtr[N], src_rowptr, scale != 0, t_build0)) {
    pa_op_shard_free(&sh); free(src_rowptr);
    return 1;
  }
  return 0;
}

int preAlps_OperatorBuildFromCSR(int N, const int* rowPtr, const int* colInd, const double* val,
                                 int nparts, const int* part, int scale) {
  return build_from_csr(N, rowPtr, colInd, val, nparts, part, scale, 1);
}

/* The MatrixMarket reader (mtx_read.c) with the host threads of this process; its reason through PA_FAIL. */
static int load_mtx(const char* file, pa_mtx_t* A) {
  char err[600];
  if (pa_mtx_read(file, pa_host_threads(), setup_trace(), A, err, sizeof(err))) return PA_FAIL("%s", err);
  return 0;
}

/* The partition vector of the whole matrix, as preAlps_OperatorBuild picks it: from
 * PREALPS_PARTITION_FILE (one part id per line, e.g. METIS output), contiguous row blocks with
 * PREALPS_PARTITION=contiguous (*part_out = NULL), else the library's k-way graph partitioner
 * (partition.c), which stands where the reference calls METIS_PartGraphKway
 * (utils/operator.c:77-97 -> utils/cplm_core/cplm_matcsr_core.c:394-457). */
static int choose_partition(int N, const int* rp, const int* ci, int nparts, int** part_out) {
  int* part = NULL;
  *part_out = NULL;
  const char* pf = getenv("PREALPS_PARTITION_FILE");
  if (pf && *pf) {
    FILE* f = fopen(pf, "r");
    if (!f) return PA_FAIL("Impossible to open the file %s", pf);
    part = (int*)malloc((size_t)N * sizeof(int));
    for (int i = 0; part && i < N; ++i)
      if (fscanf(f, "%d", &part[i]) != 1) { fclose(f); free(part); return PA_FAIL("partition file %s is too short", pf); }
    fclose(f);
    if (!part) return PA_FAIL("out of host memory");
  } else {
    const char* how = getenv("PREALPS_PARTITION");
    if (!(how && !strcmp(how, "contiguous")) && nparts > 1) {
      if (nparts > N) return PA_FAIL("invalid sizes N=%d nparts=%d", N, nparts);
      part = (int*)malloc((size_t)N * sizeof(int));
      if (!part || preAlps_hip_partition_kway(N, rp, ci, nparts, part)) { free(part); return 1; }
    }
  }
  *part_out = part;
  return 0;
}

/* rows [r0, r0 + mg) of the new order make up the panel of process g */
static void panel_rows(const pa_op_shard_t* sh, int g, int size, int* r0, int* mg) {
  const int p0 = (int)((long long)g * sh->nparts / size), p1 = (int)((long long)(g + 1) * sh->nparts / size);
  *r0 = sh->rowPos[p0]; *mg = sh->rowPos[p1] - *r0;
}

/* One MPI rank per GPU (the reference's own mode: utils/operator.c:38-134).  Rank 0 reads, scales
 * and partitions the matrix -- with the whole CPU share of the node, the other ranks sleep --
 * broadcasts the ordering and the scaling vector (12 bytes per row) and sends every rank the raw
 * rows of its panel (CPLM_MatCSRGetRowPanel + CPLM_MatCSRSend, utils/operator.c:99-108;
 * utils/cplm_light/cplm_matcsr.c:382-497); each rank then scales, renumbers and sorts its own rows,
 * finds its halo and asks the owners for exactly those rows.  No rank but 0 ever holds more than
 * its panel.
 *
 * Six stages -- header, vectors, row panels, panel build, send lists, upload -- under one rule: a rank that
 * fails records it in `rc`, skips the rest of that stage's own work and still enters every collective and
 * message of the stage, in the order of the success path; the pa_mpi_agree that closes the stage makes the
 * verdict common and every rank leaves through `done`, which releases whatever is set.  A failing pa_mpi_bcast
 * or pa_mpi_swap_lists is itself a failed collective: what the other ranks then do is beyond this rule; this
 * rank still leaves through `done`. */
static int build_distributed(const char* file, int rank, int size) {
  double t_build0 = pa_wtime();
  TRACE_DECL;
  int rc = 0, adopted = 0;
  pa_mtx_t A = {0};                         /* rank 0: the whole matrix */
  pa_op_shard_t sh = {0};
  char err[256];
  long long hdr[4] = {0, 0, 0, 0};          /* rc, N, nparts, nnz */
  long long* nzs = NULL;                    /* entries of every rank's panel */
  int* bl = NULL; int* bc = NULL; double* bv = NULL;   /* the raw rows of one panel: sent by rank 0, received by the others */
  int* asked = NULL; int* asked_cnt = NULL;
  pa_op_in_t bin = {.scale = 1, .rank = rank, .size = size, .threads = pa_host_threads(), .trace = tr};

  /* ---- header: rank 0 reads, partitions, scales and orders */
  if (rank == 0) {
    pa_host_solo(1);
    bin.threads = pa_host_threads();
    rc = load_mtx(file, &A);
    TRACE("rank 0: read the matrix");
    int nparts = env_int("PREALPS_NPARTS", size);
    int* part = NULL;
    if (!rc && (nparts < size || nparts > A.N))
      rc = PA_FAIL("Each process needs at least one block (nparts = %d, %d processes, %d rows)", nparts, size, A.N);
    rc = rc || choose_partition(A.N, A.rowPtr, A.colInd, nparts, &part);
    TRACE("rank 0: partition");
    bin.N = A.N; bin.rowPtr = A.rowPtr; bin.colInd = A.colInd; bin.val = A.val; bin.nparts = nparts; bin.part = part;
    if (!rc && pa_op_order(&bin, &sh, err, sizeof(err))) rc = PA_FAIL("%s", err);
    free(part);
    bin.part = NULL;
    pa_host_solo(0);
    bin.threads = pa_host_threads();
    hdr[0] = rc ? 1 : 0; hdr[1] = A.N; hdr[2] = nparts; hdr[3] = rc ? 0 : A.rowPtr[A.N];
  }
  if (pa_mpi_bcast(hdr, sizeof(hdr), 0)) { rc = 1; goto done; }
  if (hdr[0]) {
    if (rank != 0) rc = PA_FAIL("rank 0 could not read or partition %s", file);
    goto done;
  }
  const int N = (int)hdr[1], nparts = (int)hdr[2];

  /* ---- vectors: the ordering and the scaling vector to every rank */
  if (rank != 0) {
    bin.N = N; bin.nparts = nparts;
    sh.N = N; sh.nparts = nparts;
    sh.rowPos = (int*)malloc(((size_t)nparts + 1) * sizeof(int));
    sh.perm = (int*)malloc((size_t)N * sizeof(int));
    sh.iperm = (int*)malloc((size_t)N * sizeof(int));
    sh.d = (double*)malloc((size_t)N * sizeof(double));
    rc = !sh.rowPos || !sh.perm || !sh.iperm || !sh.d;
  }
  /* (a rank that cannot hold the vectors must not leave the others inside the broadcasts) */
  if (pa_mpi_agree(rc)) { rc = rc ? PA_FAIL("out of host memory") : PA_FAIL("another rank ran out of host memory"); goto done; }
  if (pa_mpi_bcast(sh.rowPos, ((size_t)nparts + 1) * sizeof(int), 0) || pa_mpi_bcast(sh.perm, (size_t)N * sizeof(int), 0) ||
      pa_mpi_bcast(sh.d, (size_t)N * sizeof(double), 0)) { rc = 1; goto done; }
  if (rank != 0)
    for (int k = 0; k < N; ++k) sh.iperm[sh.perm[k]] = k;
  TRACE("ordering + scaling vector (broadcast)");

  /* ---- row panels: the raw rows of every other panel travel from rank 0 -- row lengths, column ids, values,
   * three messages per rank.  The entries of every panel are announced first: every buffer of the exchange
   * exists (and the ranks have agreed that it does) before the first message, so the ranks that wait for their
   * rows hear about a failure instead of waiting for ever */
  int r0 = 0, mg = 0;                       /* this rank's rows (rank 0: the rank it is sending to) */
  panel_rows(&sh, rank, size, &r0, &mg);
  nzs = (long long*)calloc((size_t)size, sizeof(long long));
  if (pa_mpi_agree(nzs == NULL)) { rc = PA_FAIL("out of host memory"); goto done; }
  size_t cap = 0, capm = 0;                 /* rank 0: the largest panel; else: this rank's */
  if (rank == 0) {
    for (int g = 1; g < size; ++g) {
      panel_rows(&sh, g, size, &r0, &mg);
      size_t nz = 0;
      for (int i = 0; i < mg; ++i) { int old = sh.perm[r0 + i]; nz += (size_t)(A.rowPtr[old + 1] - A.rowPtr[old]); }
      if (nz > cap) cap = nz;
      if ((size_t)mg > capm) capm = (size_t)mg;
      nzs[g] = (long long)nz;
    }
    cap += 16;
  }
  if (pa_mpi_bcast(nzs, (size_t)size * sizeof(long long), 0)) { rc = rank == 0 ? 1 : PA_FAIL("receiving the panel sizes failed"); goto done; }
  if (rank != 0) { cap = (size_t)nzs[rank] ? (size_t)nzs[rank] : 1; capm = (size_t)mg; }
  bl = (int*)malloc((capm + 1) * sizeof(int));
  bc = (int*)pa_big_alloc(cap * sizeof(int));
  bv = (double*)pa_big_alloc(cap * sizeof(double));
  if (pa_mpi_agree(!bl || !bc || !bv)) {
    rc = rank == 0 ? PA_FAIL("out of host memory for the row panels")
                   : PA_FAIL("out of host memory for the row panels (%zu entries here)", (size_t)nzs[rank]);
    goto done;
  }
  if (rank == 0) {
    const int* rp = A.rowPtr;
    for (int g = 1; g < size; ++g) {
      panel_rows(&sh, g, size, &r0, &mg);
      const size_t nz = (size_t)nzs[g];
      bl[0] = 0;
      for (int i = 0; i < mg; ++i) { int old = sh.perm[r0 + i]; bl[i + 1] = bl[i] + (rp[old + 1] - rp[old]); }
#pragma omp parallel for num_threads(pa_host_threads()) schedule(static)
      for (int i = 0; i < mg; ++i) {
        int old = sh.perm[r0 + i];
        memcpy(bc + bl[i], A.colInd + rp[old], (size_t)(rp[old + 1] - rp[old]) * sizeof(int));
        memcpy(bv + bl[i], A.val + rp[old], (size_t)(rp[old + 1] - rp[old]) * sizeof(double));
      }
      /* (after a failed send the other ranks still get their rows: none of them waits in vain) */
      if (pa_mpi_send(bl, ((size_t)mg + 1) * sizeof(int), g, 41) || pa_mpi_send(bc, nz * sizeof(int), g, 42) ||
          pa_mpi_send(bv, nz * sizeof(double), g, 43))
        rc = 1;
    }
    TRACE("rank 0: panels sent");
  } else {
    const size_t nz = (size_t)nzs[rank];
    if (pa_mpi_recv(bl, ((size_t)mg + 1) * sizeof(int), 0, 41) || (size_t)bl[mg] != nz) rc = PA_FAIL("receiving the panel failed");
    if (pa_mpi_recv(bc, nz * sizeof(int), 0, 42)) rc = 1;
    if (pa_mpi_recv(bv, nz * sizeof(double), 0, 43)) rc = 1;
    TRACE("panel received");
  }

  /* ---- panel build: every rank scales, renumbers and sorts its own rows */
  if (!rc) {
    if (rank == 0) { free(bl); free(bc); free(bv); bl = NULL; bc = NULL; bv = NULL; }
    else { bin.rowPtr = bl; bin.colInd = bc; bin.val = bv; }
    if (pa_op_panel(&bin, &sh, rank == 0, 0, err, sizeof(err))) rc = PA_FAIL("%s", err);
    pa_mtx_free(&A);
    free(bl); free(bc); free(bv); bl = NULL; bc = NULL; bv = NULL;
  }
  if (pa_mpi_agree(rc)) { if (!rc) rc = PA_FAIL("another rank could not build its row panel"); goto done; }

  /* ---- send lists: every rank asks the owners for the rows behind its halo slots (halo_cols is
   * ascending, hence grouped by owner); what a rank is asked for, in that order, is what it packs */
  asked_cnt = (int*)calloc((size_t)size, sizeof(int));
  if (pa_mpi_agree(asked_cnt == NULL)) { rc = PA_FAIL("out of host memory"); goto done; }
  if (pa_mpi_swap_lists(sh.halo_cols, sh.recv_by_proc, &asked, asked_cnt)) { rc = 1; goto done; }
  {
    long long tot = 0;
    for (int g = 0; g < size; ++g) tot += asked_cnt[g];
    for (long long k = 0; k < tot; ++k) {
      int r = asked[k] - sh.row_off;
      if (r < 0 || r >= sh.m) { rc = PA_FAIL("a neighbour asked for row %d, which this rank does not own", asked[k]); break; }
      asked[k] = r;
    }
  }
  if (!rc) {
    if (pa_op_finish_peers(&sh, size, asked, asked_cnt, err, sizeof(err))) rc = PA_FAIL("%s", err);
    asked = NULL;   /* (taken over) */
  }
  TRACE("peer lists (exchanged)");

  /* ---- upload, and the shard becomes the operator (every rank holds the whole scaling vector) */
  if (!rc) { rc = adopt_shard(&g_op, &sh, size, hdr[3], NULL, 0, t_build0); adopted = !rc; }
  /* every rank leaves with the same answer: the solver's collectives come next */
  if (pa_mpi_agree(rc)) {
    if (!rc) rc = PA_FAIL("another rank could not finish its part of the operator");
    if (adopted) preAlps_OperatorFree();
  }
done:
  pa_mtx_free(&A);
  pa_op_shard_free(&sh);
  free(nzs); free(bl); free(bc); free(bv); free(asked); free(asked_cnt);
  return rc ? 1 : 0;
}

/* The number of subdomains is PREALPS_NPARTS (default: the process count, as in the
 * reference).  Started by an MPI launcher (the reference driver: MPI_Init, then
 * preAlps_OperatorBuild(file, MPI_COMM_WORLD)), rank and size come from `comm`, the device from
 * the rank's position on its node, the process-group hooks bind to RCCL (or to MPI through the
 * host when ranks share a device) and the set-up is distributed from rank 0: no caller change
 * (mpi_glue.c).  PREALPS_PLAN_ONLY=1: plan the sharding without touching a GPU. */
int preAlps_OperatorBuild(const char* matrixFilename, MPI_Comm comm) {
  size_t len = strlen(matrixFilename);
  if (len < 3 || strcmp(matrixFilename + len - 3, "mtx") != 0)
    return PA_FAIL("Only MatrixMarket (.mtx) files are supported: %s", matrixFilename);
  if (env_int("PREALPS_PLAN_ONLY", 0)) g_plan_only = 1;
  int mrank = 0, msize = 1;
  const int att = pa_mpi_attach(comm, &mrank, &msize);
  if (att < 0) return 1;       /* (an MPI this library cannot speak to: never go on as a lone process) */
  if (att) {
    if (g_op.info.built) preAlps_OperatorFree();
    if (preAlps_hip_set_world(mrank, msize)) return 1;
    if (!g_plan_only && pa_mpi_bind()) return 1;
    return build_distributed(matrixFilename, mrank, msize);
  }
  pa_mtx_t A;
  TRACE_DECL;
  if (load_mtx(matrixFilename, &A)) return 1;
  TRACE("read the matrix");
  int nparts = env_int("PREALPS_NPARTS", pa_world_size());
  int* part = NULL;
  int rc = choose_partition(A.N, A.rowPtr, A.colInd, nparts, &part);
  rc = rc || build_from_csr(A.N, A.rowPtr, A.colInd, A.val, nparts, part, 1, 0);
  free(part); pa_mtx_free(&A);
  return rc;
}

/* -------------------------------------------------------------- getters ---- */
int preAlps_OperatorGetSizes(int* M, int* m) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  *M = g_op.info.N; *m = g_op.info.m;
  return 0;
}
int preAlps_OperatorGetA(CPLM_Mat_CSR_t* A) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  *A = g_op.info.A; /* shallow view, library-owned (operator.c:353-359) */
  return 0;
}
int preAlps_OperatorGetRowPosPtr(int** rowPos, int* sizeRowPos) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  *rowPos = g_op.info.rowPos; *sizeRowPos = g_op.info.nparts + 1;
  return 0;
}
/* The reference's colPos is an O(m * P) table that only its own SpMM and
 * GetDiagBlock consume; here the row blocks carry that information, so the
 * getter hands back a one-entry placeholder that BlockJacobiCreate ignores. */
int preAlps_OperatorGetColPosPtr(int** colPos, int* sizeColPos) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  if (!g_op.colPos_dummy) g_op.colPos_dummy = (int*)calloc(1, sizeof(int));
  *colPos = g_op.colPos_dummy; *sizeColPos = 1;
  return 0;
}
int preAlps_OperatorGetDepPtr(int** dep, int* sizeDep) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  *dep = g_op.peers; *sizeDep = g_op.npeers;
  return 0;
}
/* The halo plan of this process: peers[i] receives send_rows[i] of our rows
 * (local indices in send_idx, peer after peer) and owns recv_rows[i] of our
 * halo slots (global rows in halo_cols, ascending, peer after peer). */
int preAlps_OperatorGetHaloPlan(int* npeers, int** peers, int** send_rows, int** recv_rows,
                                int** send_idx, int* nsend, int** halo_cols, int* nhalo) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  *npeers = g_op.npeers; *peers = g_op.peers; *send_rows = g_op.send_rows; *recv_rows = g_op.recv_rows;
  *send_idx = g_op.send_idx; *nsend = g_op.nsend; *halo_cols = g_op.halo_cols; *nhalo = g_op.info.halo;
  return 0;
}
int preAlps_OperatorGetPermPtr(int** perm, int* n) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  *perm = g_op.info.perm; *n = g_op.info.N;
  return 0;
}
int preAlps_OperatorGetScalingPtr(double** d, int* n) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  if (!d || !n) return PA_FAIL(" wrong test 'd != NULL && n != NULL'");
  *d = g_op.info.scaling; *n = g_op.info.N;
  return 0;
}
/* The caller's rows this process owns, in the operator's local order: the slice of the permutation the row map is cut from. */
int preAlps_OperatorGetOwnedRows(int** rows, int* m) {
  if (!g_op.info.built) return PA_FAIL("operator not built");
  if (!rows || !m) return PA_FAIL(" wrong test 'rows != NULL && m != NULL'");
  *rows = g_op.info.perm + g_op.info.row_off; *m = g_op.info.m;
  return 0;
}
/* The device copy of the row map, cut at the first system solve and again when the values (and so d) have moved. */
int pa_operator_system_map(const int** src, const double** dl) {
  pa_operator_t* o = &g_op;
  const pa_operator_info_t* in = &o->info;
  if (!in->built) return PA_FAIL("operator not built");
  if (g_plan_only) return PA_FAIL("the operator was built in plan-only mode (no GPU)");
  if (o->d_sys_src && o->sys_map_epoch == o->values_epoch) { *src = o->d_sys_src; *dl = o->d_sys_dl; return 0; }
  const size_t mm = (size_t)(in->m > 0 ? in->m : 1);
  double* hdl = (double*)malloc(mm * sizeof(double));
  if (!hdl) return PA_FAIL("out of host memory for the row map");
  const int* hsrc = in->perm + in->row_off;
  for (int i = 0; i < in->m; ++i) hdl[i] = in->scaling ? in->scaling[hsrc[i]] : 1.0;
  if (!o->d_sys_src) {
    o->d_sys_src = (int*)pa_rt_malloc(mm * sizeof(int));
    o->d_sys_dl = (double*)pa_rt_malloc(mm * sizeof(double));
  }
  int rc = !o->d_sys_src || !o->d_sys_dl || pa_rt_h2d(o->d_sys_src, hsrc, (size_t)in->m * sizeof(int)) ||
           pa_rt_h2d(o->d_sys_dl, hdl, (size_t)in->m * sizeof(double));
  free(hdl);
  if (rc) {
    pa_rt_free(o->d_sys_src); pa_rt_free(o->d_sys_dl); o->d_sys_src = NULL; o->d_sys_dl = NULL;
    return PA_FAIL("the row map of the system solve: %s", pa_rt_error());
  }
  o->sys_map_epoch = o->values_epoch;
  ++o->sys_map_builds;
  *src = o->d_sys_src; *dl = o->d_sys_dl;
  return 0;
}
int preAlps_hip_nparts(void) { return g_op.info.built ? g_op.info.nparts : 0; }

void preAlps_OperatorPrint(int rank) {
  const pa_operator_info_t* in = &g_op.info;
  if (!in->built || rank != pa_world_rank()) return;
  printf("[%d] operator: N = %d, parts = %d (own %d..%d), local rows = %d, local nnz = %d, halo rows = %d, "
         "neighbours = %d, SpMM row blocks = %d (%d interior)\n",
         rank, in->N, in->nparts, in->part0, in->part1 - 1, in->m, g_op.lnnz, in->halo, g_op.npeers,
         g_op.plan.nblk, g_op.plan.n_interior);
}

/* ----------------------------------------------------------------- SpMM ---- */
static int ensure_halo_buffers(pa_operator_t* o, int ts) {
  if (o->info.halo == 0 && o->nsend == 0) return 0;
  if (o->buf_ts >= ts) return 0;
  pa_rt_free(o->d_sendbuf); pa_rt_free(o->d_halo);
  o->d_sendbuf = (double*)pa_rt_malloc((size_t)(o->nsend ? o->nsend : 1) * ts * sizeof(double));
  o->d_halo = (double*)pa_rt_malloc((size_t)(o->info.halo ? o->info.halo : 1) * ts * sizeof(double));
  if (!o->d_sendbuf || !o->d_halo) return PA_FAIL("halo buffers: %s", pa_rt_error());
  o->buf_ts = ts;
  return 0;
}

/* The kernel that WRITES the panel X the next preAlps_BlockOperator call will multiply (the second half of an ECG
 * iteration: the new search directions) can pack the rows the neighbours need while it has them in registers -- one
 * launch less per iteration (k_pack_rows: 5 us of the 83 us a one-of-eight shard of the headline problem takes).
 * Returns 1 and the inverse send list (row -> slots of the send buffer, rows of `ts` doubles) when this process has
 * neighbours; the operator then skips its own pack for exactly that panel pointer, once.  The caller promises that
 * nothing else writes X in between (the library's own loops, PREALPS_RCI_FUSE=1). */
/* (the inverse send list itself: pa_op_inverse_send_list, op_build.h) */
/* The same list on the host, for tests without a GPU (plan-only mode): off_out[m + 1], slot_out[nsend]. */
int preAlps_hip_pack_map(int* off_out, int* slot_out) {
  pa_operator_t* o = &g_op;
  if (!o->info.built) return PA_FAIL("operator not built");
  int m = o->info.m;
  int* off = (int*)calloc((size_t)m + 2, sizeof(int));
  if (!off) return PA_FAIL("out of host memory");
  pa_op_inverse_send_list(m, o->nsend, o->send_idx, off, slot_out);
  memcpy(off_out, off, ((size_t)m + 1) * sizeof(int));
  free(off);
  return 0;
}
static long long g_packs_fused = 0;       /* products whose send rows the solver's update kernel had packed */
int pa_operator_pack_hint(int ts, const double* X, const int** pk_off, const int** pk_slot, double** sendbuf) {
  pa_operator_t* o = &g_op;
  o->prepacked = NULL;
  if (!o->info.built || g_plan_only || pa_world_size() <= 1 || o->npeers <= 0 || o->nsend <= 0 || !X) return 0;
  if (!env_int("PREALPS_PACK_FUSE", 1)) return 0;
  if (ensure_halo_buffers(o, ts)) return 0;
  if (o->buf_ts != ts) return 0;            /* (buffers sized for a wider panel: slots would be ts_buf apart) */
  if (!o->d_pk_off) {
    int m = o->info.m;
    int* off = (int*)calloc((size_t)m + 2, sizeof(int));
    int* slot = (int*)malloc((size_t)o->nsend * sizeof(int));
    int ok = off && slot;
    if (ok) {
      pa_op_inverse_send_list(m, o->nsend, o->send_idx, off, slot);
      o->d_pk_off = (int*)pa_rt_malloc(((size_t)m + 1) * sizeof(int));
      o->d_pk_slot = (int*)pa_rt_malloc((size_t)o->nsend * sizeof(int));
      ok = o->d_pk_off && o->d_pk_slot && !pa_rt_h2d(o->d_pk_off, off, ((size_t)m + 1) * sizeof(int)) &&
           !pa_rt_h2d(o->d_pk_slot, slot, (size_t)o->nsend * sizeof(int));
      if (!ok) { pa_rt_free(o->d_pk_off); pa_rt_free(o->d_pk_slot); o->d_pk_off = o->d_pk_slot = NULL; }
    }
    free(off); free(slot);
    if (!ok) return 0;
  }
  *pk_off = o->d_pk_off; *pk_slot = o->d_pk_slot; *sendbuf = o->d_sendbuf;
  o->prepacked = X;
  return 1;
}

/* Cut the SpMM plan for a given enlarging factor now instead of at the first
 * preAlps_BlockOperator call (it is host work proportional to the local nonzeros). */
int preAlps_hip_prepare_operator(int enlFac) {
  pa_operator_t* o = &g_op;
  if (!o->info.built) return PA_FAIL("operator not built");
  if (operator_bits() < 0) return 1;      /* (what the cut itself would refuse, without a GPU as well) */
  if (g_plan_only) return 0;
  int ts = pa_panel_stride(enlFac);
  double t0 = pa_wtime();
  if (o->plan_ts != ts && build_plan(o, ts)) return 1;
  g_setup_plan_s = pa_wtime() - t0;
  return 0;
}

int pa_operator_plan_epoch(void) { return g_plan_epoch; }

/* Storage of the matrix values the products read: 64, 32, or 0 = follow PREALPS_SPMM_PRECISION.  Needs no GPU.  A plan
 * that is on the device follows at once, behind the work already queued: a packed run plan at up to 4 columns gets
 * its fp32 copy or drops it (its fp64 array stays where it is); an unpacked run plan at such a stride is cut again,
 * packed, when 32 comes into force; every other plan is left alone.  A refusal leaves the setting as it was, and the
 * plan too -- but for an unpacked run plan whose new cut failed: that plan is gone, and the next product cuts it again
 * under the old setting. */
static int recode_plan(pa_operator_t* o);
int preAlps_hip_set_operator_precision(int bits) {
  pa_operator_t* o = &g_op;
  if (bits != 0 && bits != 32 && bits != 64)
    return PA_FAIL("precision %d refused: 64 (double), 32 (single) or 0 (follow PREALPS_SPMM_PRECISION)", bits);
  const int before = g_op_bits;
  g_op_bits = bits;
  if (!o->info.built || g_plan_only || o->plan_ts == 0) return 0;
  const char* pe = getenv("PREALPS_SPMM_PRECISION");
  if (!bits && pe && *pe && strcmp(pe, "double") && strcmp(pe, "single")) return 0;   /* (the next plan cut names it) */
  const int want = operator_bits();
  const pa_spmm_plan_t* pl = &o->plan;
  if (want != 32) o->val32_owed = 0;      /* (a copy that an update could not form is no longer wanted) */
  if ((want == 32) == (pl->val32 != NULL)) return 0;
  if (pa_rt_sync()) { g_op_bits = before; return PA_FAIL("%s", pa_rt_error()); }   /* products in flight read the plan */
  if (want == 64) {
    drop_val32(o);
    /* (fp64 again: the codes, which went when the float copy came, are formed anew where the rule holds) */
    if (pl->packed && !pl->coded && o->plan_code_sw != 0 && (o->plan_ts == 2 || o->plan_ts == 4)) return recode_plan(o);
    return 0;
  }
  if (!pl->runs || pl->runs_cols != o->plan_ts || o->plan_ts > 4 || o->plan_pack_sw == 0) return 0;
  if (pl->packed ? form_val32(o) : build_plan(o, o->plan_ts)) { g_op_bits = before; o->val32_owed = 0; return 1; }
  if (o->plan.coded) { free_codes(o); ++g_plan_epoch; }      /* (no codes beside the float copy) */
  return 0;
}

/* ------------------------------------------------------ new values in place ---- */
int pa_operator_values_epoch(void) { return g_op.values_epoch; }
int pa_operator_plan_stride(void) { return g_op.plan_ts; }
int pa_operator_build_count(void) { return g_op_builds; }
/* the last update: host seconds of scaling vector + panel, host seconds of the copy of the panel values to the
 * device, device seconds of k_plan_set_values between two events; the seconds the last value map took (cut, upload) */
static double g_update_host_s, g_update_copy_s, g_update_kernel_s, g_update_map_s;

/* The value map of the current plan on the device, cut once per plan (spmm_plan.h). */
static int ensure_value_map(pa_operator_t* o) {
  if (o->d_vmap) return 0;
  pa_spmm_plan_in_t pin = plan_input(o, o->plan_ts);
  pa_spmm_value_map_t vm;
  if (pa_spmm_plan_value_map(&pin, &vm)) return PA_FAIL("out of host memory for the value map of the SpMM plan");
  ++o->vmap_builds;
  int rc = 0;
  if (vm.nslices != o->plan.nslices || vm.nblk != o->plan.nblk || vm.staged != o->plan.staged || vm.runs != o->plan.runs ||
      vm.runs_cols != o->plan.runs_cols || vm.n != o->plan_val_n)
    rc = PA_FAIL("the value map does not fit the SpMM plan on the device (slices %d / %d, blocks %d / %d, values %zu / %zu)",
                 vm.nslices, o->plan.nslices, vm.nblk, o->plan.nblk, vm.n, o->plan_val_n);
  if (!rc) {
    unsigned* dm = (unsigned*)pa_rt_malloc((vm.n ? vm.n : 1) * sizeof(unsigned));
    if (!dm || pa_rt_h2d(dm, vm.map, vm.n * sizeof(unsigned))) {
      pa_rt_free(dm);
      rc = PA_FAIL("uploading the value map failed: %s", pa_rt_error());
    } else o->d_vmap = dm;
  }
  free(vm.map);
  return rc;
}

/* The packed values of the current run plan anew, from the host panel as it stands: the plan a build would cut
 * for it (the same slices, slots and blocks: no decision of a builder reads a value), packed and uploaded into
 * fresh arrays; the old ones go only when the new ones are on the device. */
static int repack_plan(pa_operator_t* o) {
  pa_spmm_plan_in_t pin = plan_input(o, o->plan_ts);
  pa_spmm_host_plan_t hp;
  if (pa_spmm_plan_build(&pin, &hp)) return PA_FAIL("out of host memory for the SpMM plan");
  pa_spmm_pack_t pk;
  int rc = 0;
  if (!hp.runs || hp.nslices != o->plan.nslices || hp.a[PA_PL_VAL].n != o->plan_val_n) {
    pa_spmm_plan_free(&hp);
    return PA_FAIL("the SpMM plan cut for the new values does not fit the plan on the device");
  }
  if (pa_spmm_pack_build((const double*)hp.a[PA_PL_VAL].p, (const long long*)hp.a[PA_PL_SL_OFF].p,
                         (const int*)hp.a[PA_PL_SL_LEN].p, hp.nslices, 0, &pk)) {
    pa_spmm_plan_free(&hp);
    return PA_FAIL("out of host memory for the packed values of the SpMM plan");
  }
  void *d_val = NULL, *d_meta = NULL;
  if (upload_pack(&pk, &d_val, &d_meta)) rc = PA_FAIL("uploading the packed values failed: %s", pa_rt_error());
  else {
    pa_rt_free(o->d_plan[PA_PL_VAL]); pa_rt_free((void*)o->plan.pk_meta);
    o->d_plan[PA_PL_VAL] = d_val; o->plan.val = (const double*)d_val;
    o->plan.pk_meta = (const unsigned long long*)d_meta;
    o->pk_nval = pk.nval;
    o->pk_stream_bytes = hp.stream_bytes - pk.unpacked_bytes + pk.packed_bytes;
    g_dbg_val_bytes = pk.nval_alloc * sizeof(double);
    ++o->repacks;
    ++g_plan_epoch;
    /* the fp32 copy follows the new array: another length, so another allocation */
    const int had32 = o->plan.val32 != NULL;
    drop_val32(o);
    o->pk_nalloc = pk.nval_alloc;
    if (had32) rc = form_val32(o);
    /* the codes of the old array do not fit the new one: formed anew where the rule still holds, else dropped */
    const int was_coded = o->plan.coded;
    if (was_coded) { free_codes(o); ++g_plan_epoch; }
    if (!rc && !o->plan.val32) {
      rc = code_plan(o, &hp, &pk, o->plan_ts, operator_bits());
      if (!rc && (was_coded || o->plan.coded)) ++o->recodes;
    }
  }
  pa_spmm_pack_free(&pk);
  pa_spmm_plan_free(&hp);
  return rc;
}

/* The codes of the packed array as it stands on the device, anew: the plan a build would cut for the host panel,
 * packed and coded on the host (the path of repack_plan), the codes uploaded; the packed array is not touched.  The
 * caller has made sure that no new value lacks a place (k_pack_set_values), so the fresh pack has the layout of the
 * array on the device exactly when it keeps as many values; when a kept place now holds +0.0 it keeps fewer, and the
 * codes are dropped: the products read fp64 until the next build or repack.  (Writing the codes through on the device
 * would spare the host pass: not done here.) */
static int recode_plan(pa_operator_t* o) {
  pa_spmm_plan_in_t pin = plan_input(o, o->plan_ts);
  pa_spmm_host_plan_t hp;
  if (pa_spmm_plan_build(&pin, &hp)) { free_codes(o); ++g_plan_epoch; return PA_FAIL("out of host memory for the SpMM plan"); }
  pa_spmm_pack_t pk;
  int rc = 0;
  if (!hp.runs || hp.nslices != o->plan.nslices || hp.a[PA_PL_VAL].n != o->plan_val_n ||
      pa_spmm_pack_build((const double*)hp.a[PA_PL_VAL].p, (const long long*)hp.a[PA_PL_SL_OFF].p,
                         (const int*)hp.a[PA_PL_SL_LEN].p, hp.nslices, 0, &pk)) {
    pa_spmm_plan_free(&hp);
    free_codes(o); ++g_plan_epoch;
    return PA_FAIL("the SpMM plan cut for the new values does not fit the plan on the device");
  }
  if (pk.nval != o->pk_nval || pk.nval_alloc != o->pk_nalloc) { free_codes(o); ++g_plan_epoch; }
  else if ((rc = code_plan(o, &hp, &pk, o->plan_ts, operator_bits())) != 0) { free_codes(o); ++g_plan_epoch; }   /* (never stale codes) */
  if (!rc) ++o->recodes;
  pa_spmm_pack_free(&pk);
  pa_spmm_plan_free(&hp);
  return rc;
}

/* The operator that a fresh preAlps_OperatorBuildFromCSR with these values (same pattern, partition and scale) would
 * give, bit for bit, without the build: the host panel is rewritten through o->src, the plan on the device through
 * its value map (k_plan_set_values); every address stays.  Every refusal and every allocation comes before the first
 * write.  A packed run plan (spmm_pack.h) is written through its masks (k_pack_set_values); only when a value that
 * the pack dropped as +0.0 becomes something else are the values packed anew, into new arrays (repack_plan).  A plan
 * that holds codes (spmm_code.h) gets them anew from the host panel after the write, or loses them (recode_plan). */
int preAlps_OperatorUpdateValues(const double* val) {
  pa_operator_t* o = &g_op;
  pa_operator_info_t* in = &o->info;
  if (!in->built) return PA_FAIL("operator not built");
  if (!o->from_csr)
    return PA_FAIL("the operator was built from a file by preAlps_OperatorBuild: the order of its values is not the caller's");
  if (!val) return PA_FAIL(" wrong test 'val != NULL'");
  double t0 = pa_wtime();
  g_update_copy_s = g_update_kernel_s = 0.0;
  const int N = in->N;
  double* d = NULL;
  if (o->scaled && !in->scaling) return PA_FAIL("the operator is scaled but holds no scaling vector");
  if (o->scaled) {   /* the scaling vector of the build, from the new values */
    d = (double*)malloc((size_t)N * sizeof(double));
    if (!d) return PA_FAIL("out of host memory");
    if (pa_op_scaling(N, o->src_rowptr, val, pa_host_threads(), d)) { free(d); return PA_FAIL("Impossible to scale the matrix, rcmin=0"); }
  }
  const int on_device = !g_plan_only && o->plan_ts != 0;
  double* d_pv = NULL;
  unsigned* d_miss = NULL;
  if (on_device) {
    double tm = pa_wtime();
    const int cut = !o->d_vmap;
    if (ensure_value_map(o)) { free(d); return 1; }
    if (cut) g_update_map_s = pa_wtime() - tm;
    t0 += pa_wtime() - tm;
    d_pv = (double*)pa_rt_malloc((size_t)(o->lnnz ? o->lnnz : 1) * sizeof(double));
    if (!d_pv) { free(d); return PA_FAIL("no device memory for the new panel values: %s", pa_rt_error()); }
    if (o->plan.packed) {
      d_miss = (unsigned*)pa_rt_malloc(sizeof(unsigned));
      if (!d_miss) { free(d); pa_rt_free(d_pv); return PA_FAIL("no device memory for the update of the packed plan: %s", pa_rt_error()); }
    }
  }
  /* the panel, as the build forms it (pa_op_panel_value) */
  const CPLM_Mat_CSR_t* A = &in->A;
  pa_op_panel_values(in->m, in->row_off, A->rowPtr, A->colInd, o->src, in->perm, d, val, pa_host_threads(), A->val);
  /* the last refusal is behind us: the new vector into the allocation the getter handed out */
  if (d) memcpy(in->scaling, d, (size_t)N * sizeof(double));
  free(d);
  ++o->values_epoch;
  g_update_host_s = pa_wtime() - t0;
  if (!on_device) return 0;
  /* behind the products already queued on the library stream; the copy returns when it has read A->val */
  t0 = pa_wtime();
  int rc = pa_rt_h2d(d_pv, A->val, (size_t)o->lnnz * sizeof(double));
  g_update_copy_s = pa_wtime() - t0;
  void* e0 = pa_rt_event_create();
  void* e1 = pa_rt_event_create();
  if (o->plan.packed) {
    /* the packed values have places only for what was not +0.0: count first what has none, write nothing */
    unsigned misses = 0;
    rc = rc || !e0 || !e1 || pa_rt_event_record(e0) || pa_rt_memset(d_miss, 0, sizeof(unsigned)) ||
         pa_k_pack_set_values(o->d_vmap, d_pv, o->plan.pk_meta, (double*)o->plan.val, o->plan_val_n, 0, d_miss) ||
         pa_rt_d2h(&misses, d_miss, sizeof(unsigned));
    if (!rc && misses) {
      /* a dropped place receives a value: pack anew, from the plan a fresh build would cut; the address moves */
      pa_rt_event_destroy(e0); pa_rt_event_destroy(e1);
      pa_rt_free(d_pv); pa_rt_free(d_miss);
      return repack_plan(o);
    }
    rc = rc || pa_k_pack_set_values(o->d_vmap, d_pv, o->plan.pk_meta, (double*)o->plan.val, o->plan_val_n, 1, d_miss) ||
         pa_rt_event_record(e1) || pa_rt_sync();
    pa_rt_free(d_miss);
    /* the fp32 copy is rounded again from the array just written, in place */
    if (!rc && o->plan.val32 && form_val32(o)) {
      pa_rt_event_destroy(e0); pa_rt_event_destroy(e1);
      pa_rt_free(d_pv);
      return 1;
    }
    /* the codes name the old values: anew from the host panel, or gone */
    if (rc && o->plan.coded) { free_codes(o); ++g_plan_epoch; }
    if (!rc && o->plan.coded && recode_plan(o)) {
      pa_rt_event_destroy(e0); pa_rt_event_destroy(e1);
      pa_rt_free(d_pv);
      return 1;
    }
  } else {
    rc = rc || !e0 || !e1 || pa_rt_event_record(e0) ||
         pa_k_plan_set_values(o->d_vmap, d_pv, (double*)o->plan.val, o->plan_val_n) || pa_rt_event_record(e1) || pa_rt_sync();
  }
  if (!rc) g_update_kernel_s = pa_rt_event_elapsed_s(e0, e1);
  pa_rt_event_destroy(e0); pa_rt_event_destroy(e1);
  pa_rt_free(d_pv);             /* (the launch has finished) */
  if (rc) return PA_FAIL("writing the new values into the SpMM plan failed: %s", pa_rt_error());
  return 0;
}

/* Run-to-run spread study: move the matrix values (which & 1) and / or the slot array
 * (which & 2) of the run plan to freshly allocated device memory; the old arrays stay allocated, so the
 * new ones land on other physical pages. */
int preAlps_hip_debug_move_plan(int which) {
  pa_operator_t* o = &g_op;
  if (!o->plan.runs || !g_dbg_val_bytes) return PA_FAIL("no run plan");
  if (which & 1) {
    double* nv = (double*)pa_rt_malloc(g_dbg_val_bytes);
    if (!nv || pa_rt_d2d(nv, o->plan.val, g_dbg_val_bytes) || pa_rt_sync()) return PA_FAIL("%s", pa_rt_error());
    o->d_plan[PA_PL_VAL] = nv; o->plan.val = nv;
  }
  if (which & 2) {
    unsigned short* nc = (unsigned short*)pa_rt_malloc(g_dbg_slot_bytes);
    if (!nc || pa_rt_d2d(nc, o->plan.col16, g_dbg_slot_bytes) || pa_rt_sync()) return PA_FAIL("%s", pa_rt_error());
    o->d_plan[PA_PL_COL16] = nc; o->plan.col16 = nc;
  }
  return 0;
}

int pa_operator_gram_blocks(int ts) {
  pa_operator_t* o = &g_op;
  if (!o->info.built || g_plan_only || ts != 4) return 0;
  if (o->plan_ts != ts && build_plan(o, ts)) return 0;
  /* Default: on, from absolute times of 800-iteration solves alternating in one process.  The window kernel
   * (k_spmm_gram; Poisson 100^3): 245.3 -> 236.9 us per iteration with the block (round 3, tools/probe/abs_ab.py).
   * The run kernel (k_spmm_runs_gram; elasticity 70^3): no gain in round 3 (397.0 -> 399.0 us: its epilogue and
   * the rows of R cost what k_gram and its sum cost); with round 4's kernel -- the matrix groups double-buffered,
   * so the epilogue of one wavefront runs beside the stream of the others -- 407.5 -> 398.1 us
   * (tools/probe/r4_solve_env_ab.py, profiles/r04_spmm_gram_ab.txt).  PREALPS_SPMM_GRAM=0 / 1 forces. */
  int dflt = 1;
  if (!env_int("PREALPS_SPMM_GRAM", dflt)) return 0;
  return o->plan.nblk;
}

/* AX = A X for the X->info.n current columns (operator.c:334-351).  exact: on the fp64 values whatever the storage in
 * force, and outside every Gram request (pa_operator_apply_exact). */
static int block_operator(CPLM_Mat_Dense_t* X, CPLM_Mat_Dense_t* AX, int exact) {
  pa_operator_t* o = &g_op;
  if (!o->info.built) return PA_FAIL("operator not built");
  if (g_plan_only) return PA_FAIL("the operator was built in plan-only mode (no GPU)");
  if (!X || !AX || !X->val || !AX->val) return PA_FAIL(" wrong test 'X->val != NULL && AX->val != NULL'");
  int ts = pa_desc_stride(X);
  if (pa_desc_stride(AX) != ts || X->info.m != o->info.m)
    return PA_FAIL("panel shapes do not match the operator (m %d vs %d, stride %d vs %d)", X->info.m,
                   o->info.m, ts, pa_desc_stride(AX));
  if (o->plan_ts != ts && build_plan(o, ts)) return 1;
  if (o->val32_owed && !exact) {      /* an update could not round its values: with 32 still in force, again or fail */
    if (operator_bits() != 32) o->val32_owed = 0;
    else if (form_val32(o)) return 1;
  }
  pa_time_begin(PA_T_OPERATOR);
  if (pa_world_size() > 1 && o->npeers > 0) {
    int rc = ensure_halo_buffers(o, ts);
    if (rc) return rc;
    for (int i = 0; i < o->npeers; ++i) { o->send_cnt[i] = o->send_rows[i] * ts; o->recv_cnt[i] = o->recv_rows[i] * ts; }
    /* Exchange beside the interior blocks only when those keep the device busy for longer than the
     * two cross-stream hand-overs cost (8 + 12 us of idle main stream measured around a 10 us interior
     * launch in the one-shard rehearsal): from about 12 M interior nonzeros (25 us); below that the
     * exchange runs on the main stream and one launch covers all blocks.  PREALPS_HALO_OVERLAP=0 / 1 forces. */
    static int overlap_env = -2;
    if (overlap_env == -2) overlap_env = env_int("PREALPS_HALO_OVERLAP", -1);
    int overlap = overlap_env >= 0 ? overlap_env
                                   : (double)o->lnnz * o->plan.n_interior / (o->plan.nblk > 0 ? o->plan.nblk : 1) >= 12e6;
    /* (the solver's update kernel has packed exactly this panel: pa_operator_pack_hint) */
    int packed = o->prepacked && o->prepacked == X->val && o->buf_ts == ts;
    o->prepacked = NULL;
    g_packs_fused += packed;
    if (!overlap) {
      if (!packed) PA_CHECK(pa_k_pack_rows(o->nsend, ts, o->d_send_idx, X->val, o->d_sendbuf));
      rc = pa_exchange(o->d_sendbuf, o->send_cnt, o->d_halo, o->recv_cnt, o->peers, o->npeers);
      if (rc) return rc;
      PA_CHECK(pa_k_spmm(&o->plan, ts, X->val, o->d_halo, AX->val, 2, exact));
      pa_time_end(PA_T_OPERATOR);
      return 0;
    }
    if (!o->ev_packed) { o->ev_packed = pa_rt_event_create(); o->ev_halo = pa_rt_event_create(); }
    if (!o->ev_packed || !o->ev_halo) return PA_FAIL("hipEventCreate failed");
    /* pack on the main stream; the exchange runs on the side stream while the main stream
     * computes the blocks that read no halo row; the halo-reading blocks wait for it */
    void* main_stream = pa_rt_stream();
    void* side = pa_rt_side_stream();
    if (!packed) PA_CHECK(pa_k_pack_rows(o->nsend, ts, o->d_send_idx, X->val, o->d_sendbuf));
    PA_CHECK(pa_rt_event_record_on(o->ev_packed, main_stream));
    PA_CHECK(pa_rt_stream_wait_event(side, o->ev_packed));
    pa_rt_set_stream(side);
    rc = pa_exchange(o->d_sendbuf, o->send_cnt, o->d_halo, o->recv_cnt, o->peers, o->npeers);
    int rc2 = rc ? 0 : pa_rt_event_record_on(o->ev_halo, side);
    pa_rt_set_stream(main_stream);
    if (rc) return rc;
    if (rc2) return PA_FAIL("%s", pa_rt_error());
    PA_CHECK(pa_k_spmm(&o->plan, ts, X->val, o->d_halo, AX->val, 0, exact));
    PA_CHECK(pa_rt_stream_wait_event(main_stream, o->ev_halo));
    PA_CHECK(pa_k_spmm(&o->plan, ts, X->val, o->d_halo, AX->val, 1, exact));
  } else {
    PA_CHECK(pa_k_spmm(&o->plan, ts, X->val, NULL, AX->val, 2, exact));
  }
  pa_time_end(PA_T_OPERATOR);
  return 0;
}

int preAlps_BlockOperator(CPLM_Mat_Dense_t* X, CPLM_Mat_Dense_t* AX) { return block_operator(X, AX, 0); }
/* The product of a start from a guess (ecg_start.c): R0 = b - A x0 is formed with the matrix as the caller gave it. */
int pa_operator_apply_exact(CPLM_Mat_Dense_t* X, CPLM_Mat_Dense_t* AX) { return block_operator(X, AX, 1); }

int preAlps_hip_get_stat(const char* key, double* value) {
  const pa_operator_t* o = &g_op;
  if (!strcmp(key, "nnz_local")) *value = o->lnnz;
  else if (!strcmp(key, "rows_local")) *value = o->info.m;
  else if (!strcmp(key, "halo_rows")) *value = o->info.halo;
  else if (!strcmp(key, "send_rows")) *value = o->nsend;
  else if (!strcmp(key, "spmm_blocks")) *value = o->plan.nblk;
  else if (!strcmp(key, "spmm_gram_launches")) *value = (double)pa_k_spmm_gram_launches();
  else if (!strcmp(key, "bj_gram_applies")) *value = (double)pa_k_bj_gram_applies();
  else if (!strcmp(key, "ecg_graph_captures")) *value = (double)pa_ecg_graph_count(0);
  else if (!strcmp(key, "ecg_graph_replays")) *value = (double)pa_ecg_graph_count(1);
  else if (!strcmp(key, "ecg_x_skips")) *value = (double)pa_ecg_x_count(0);
  else if (!strcmp(key, "ecg_x_flushes")) *value = (double)pa_ecg_x_count(1);
  else if (!strcmp(key, "ecg_energy_launches")) *value = (double)pa_ecg_energy_count();
  else if (!strcmp(key, "packs_fused")) *value = (double)g_packs_fused;
  else if (!strcmp(key, "allreduces")) *value = (double)pa_allreduce_count();
  else if (!strcmp(key, "spmm_slices")) *value = o->plan.nslices;
  else if (!strcmp(key, "spmm_stored_entries")) *value = o->sell_entries;
  else if (!strcmp(key, "spmm_stream_bytes")) *value = o->stream_bytes;
  else if (!strcmp(key, "spmm_packed")) *value = o->plan.packed;      /* the values are on the device without their zeros */
  else if (!strcmp(key, "spmm_packed_values")) *value = (double)o->pk_nval;
  else if (!strcmp(key, "spmm_packed_stream_bytes")) *value = o->pk_stream_bytes;
  else if (!strcmp(key, "spmm_repacks")) *value = o->repacks;
  else if (!strcmp(key, "spmm_precision")) *value = o->plan_ts ? (o->plan.val32 ? 32 : 64) : 0;      /* storage the products of the plan in use read */
  else if (!strcmp(key, "spmm_val32_bytes")) *value = o->plan.val32 ? 4.0 * (double)o->pk_nalloc : 0.0;
  else if (!strcmp(key, "spmm_val32_address")) *value = (double)(uintptr_t)o->plan.val32;
  else if (!strcmp(key, "spmm_precision_stream_bytes"))      /* what one product streams: 4 bytes less per packed value and step zero */
    *value = !o->plan_ts ? 0.0 : o->plan.val32 ? o->pk_stream_bytes - 4.0 * (double)(o->pk_nalloc - PA_SPMM_PACK_SLACK)
                                               : o->plan.packed ? o->pk_stream_bytes : o->stream_bytes;
  /* (spmm_precision_stream_bytes prices the storage precision alone, as its tests hold it; what a coded product
   * streams is spmm_coded_stream_bytes) */
  else if (!strcmp(key, "spmm_coded")) *value = o->plan.coded;      /* the products read 2-byte codes and per-block tables */
  else if (!strcmp(key, "spmm_coded_blocks")) *value = o->code_blocks;
  else if (!strcmp(key, "spmm_code_table_entries")) *value = (double)o->code_entries;
  else if (!strcmp(key, "spmm_coded_stream_bytes")) *value = o->code_stream_bytes;
  else if (!strcmp(key, "spmm_recodes")) *value = o->recodes;
  else if (!strcmp(key, "spmm_code_lds_bytes")) *value = o->plan.code_lds;
  else if (!strcmp(key, "spmm_round_kernel_s")) *value = g_round_kernel_s;
  else if (!strcmp(key, "spmm_val_address")) *value = (double)(uintptr_t)o->plan.val;      /* (for the run-to-run spread study) */
  else if (!strcmp(key, "spmm_slot_address")) *value = (double)(uintptr_t)o->plan.col16;
  else if (!strcmp(key, "spmm_staged")) *value = o->plan.staged;
  else if (!strcmp(key, "spmm_runs")) *value = o->plan.runs;
  else if (!strcmp(key, "spmm_stage_rows")) *value = o->plan.stage_cap;
  else if (!strcmp(key, "spmm_interior_blocks")) *value = o->plan.n_interior;
  else if (!strcmp(key, "op_values_epoch")) *value = o->values_epoch;
  else if (!strcmp(key, "op_value_map_builds")) *value = o->vmap_builds;
  else if (!strcmp(key, "op_value_map_bytes")) *value = o->d_vmap ? (double)o->plan_val_n * sizeof(unsigned) : 0.0;
  else if (!strcmp(key, "op_system_map_builds")) *value = o->sys_map_builds;
  else if (!strcmp(key, "op_system_map_bytes")) *value = o->d_sys_src ? 12.0 * (double)o->info.m : 0.0;
  else if (!strcmp(key, "bj_values_epoch")) *value = pa_bj_values_epoch();
  else if (!strcmp(key, "op_update_host_s")) *value = g_update_host_s;
  else if (!strcmp(key, "op_update_copy_s")) *value = g_update_copy_s;
  else if (!strcmp(key, "op_update_kernel_s")) *value = g_update_kernel_s;
  else if (!strcmp(key, "op_update_map_s")) *value = g_update_map_s;
  else if (!strcmp(key, "setup_build_s")) *value = g_setup_build_s;
  else if (!strcmp(key, "setup_plan_s")) *value = g_setup_plan_s;
  else if (!strcmp(key, "setup_bj_factor_s")) *value = pa_bj_setup_seconds(0);
  else if (!strcmp(key, "setup_bj_layout_s")) *value = pa_bj_setup_seconds(1);
  else if (!strcmp(key, "bj_factor_bytes")) *value = pa_bj_factor_bytes();
  else if (!strcmp(key, "bj_max_bandwidth")) *value = pa_bj_max_bandwidth();
  else if (!strcmp(key, "bj_parts_local")) *value = pa_bj_nparts();
  else if (!strcmp(key, "bj_nd_blocks")) *value = pa_bj_nd_blocks();
  else if (!strcmp(key, "bj_pairs_bytes")) *value = pa_bj_pairs_bytes();
  else if (!strcmp(key, "bj_g4_bytes")) *value = pa_bj_g4_bytes();
  else if (!strcmp(key, "bj_nd_inverse_dev")) *value = pa_nd_inverse_deviation();
  else if (!strcmp(key, "bj_nd_precision")) *value = pa_bj_nd_precision();
  else if (!strcmp(key, "bj_band_precision")) *value = pa_bj_band_precision();
  else if (!strcmp(key, "bj_g4_last_ring")) *value = pa_bj_g4_last(0);
  else if (!strcmp(key, "bj_g4_last_bits")) *value = pa_bj_g4_last(1);
  else if (!strcmp(key, "bj_g4_last_pipelined")) *value = pa_bj_g4_last(2);
  else if (!strcmp(key, "bj_g4_last_paired")) *value = pa_bj_g4_last(3);
  else if (!pa_hist_stat(key, value)) return 0;
  else return pa_bj_update_stat(key, value);
  return 0;
}

/* rhs of examples/test_ecg_prealps_op.c:172-184 as np = nparts ranks build it:
 * every rank restarts the generator (srand(0)), the 2-norm is global, and
 * element 0 of every rank is left unscaled. */
int preAlps_hip_reference_rhs(double* rhs_local) {
  const pa_operator_info_t* in = &g_op.info;
  if (!in->built) return PA_FAIL("operator not built");
  int mmax = 0;
  for (int p = 0; p < in->nparts; ++p) { int l = in->rowPos[p + 1] - in->rowPos[p]; if (l > mmax) mmax = l; }
  double* stream = (double*)malloc((size_t)(mmax > 0 ? mmax : 1) * sizeof(double));
  if (!stream) return PA_FAIL("out of host memory");
  srand(0);
  for (int i = 0; i < mmax; ++i) stream[i] = ((double)rand() / (double)RAND_MAX);
  double normb = 0.0;
  for (int p = 0; p < in->nparts; ++p) {
    int l = in->rowPos[p + 1] - in->rowPos[p];
    double s = 0.0;
    for (int i = 0; i < l; ++i) s += stream[i] * stream[i];
    normb += s;
  }
  normb = sqrt(normb);
  for (int p = in->part0; p < in->part1; ++p) {
    int base = in->rowPos[p] - in->row_off, l = in->rowPos[p + 1] - in->rowPos[p];
    rhs_local[base] = stream[0];
    for (int i = 1; i < l; ++i) rhs_local[base + i] = stream[i] / normb;
  }
  free(stream);
  return 0;
}
