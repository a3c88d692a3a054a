/*
 * pa_device.h -- the thin C-ABI shim between the C host code (ecg.c,
 * operator.c, block_jacobi.c) and the HIP side (runtime.hip, dense_*.hip,
 * bj_band.hip, ...).
 * Host code never includes a HIP header; device code never sees a preAlps
 * struct.  Panels are row-interleaved: element (i, j) at p[i * ts + j].
 */
#ifndef PA_DEVICE_H
#define PA_DEVICE_H
#include <stddef.h>
#include "bj_g4_plan.h"    /* pa_bj_g4_max_rows / _max_band / _max_band8: the limits of the band block solve */
#include "bj_band_plan.h"  /* pa_bj_max_R, pa_bj_factor_wmax: the limits of the other band kernels */
#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime (runtime.hip) --------------------------------------------- */
int pa_rt_init(int device);
void pa_rt_shutdown(void);
int pa_rt_ready(void);
void pa_rt_set_stream(void* s);
void* pa_rt_stream(void);
int pa_rt_sync(void);
const char* pa_rt_error(void);
/* The one error text of the device side: the runtime calls and every kernel unit (a launcher that refuses its
 * arguments, a failed launch) leave their reason here, where PA_CHECK and the host's pa_rt_error() calls read it. */
void pa_rt_set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void* pa_rt_malloc(size_t bytes);
void pa_rt_free(void* d);
void* pa_rt_host_alloc(size_t bytes);
void* pa_rt_host_alloc_coherent(size_t bytes);   /* fine-grained: a kernel writes, the host polls */
int pa_rt_stream_state(void);                     /* 0: work pending, 1: idle, -1: error */
void pa_rt_host_free(void* h);
int pa_rt_memset(void* d, int v, size_t bytes);
int pa_rt_h2d(void* d, const void* h, size_t bytes);
int pa_rt_d2h(void* h, const void* d, size_t bytes);
int pa_rt_d2d(void* dst, const void* src, size_t bytes);
int pa_rt_h2d_async(void* d, const void* pinned, size_t bytes);
int pa_rt_d2h_async(void* pinned, const void* d, size_t bytes);
void* pa_rt_side_stream(void);
int pa_rt_stream_wait_event(void* stream, void* event);
int pa_rt_event_record_on(void* event, void* stream);
void* pa_rt_event_create(void);
void pa_rt_event_destroy(void* e);
int pa_rt_event_record(void* e);
int pa_rt_event_wait(void* e);
double pa_rt_event_elapsed_s(void* a, void* b);
int pa_rt_num_cus(void);
int pa_rt_device_count(void);
/* graphs (runtime.hip): capture the work queued on the current stream, replay it later */
int pa_rt_capture_begin(void);
int pa_rt_capture_end(void** exec_out);
int pa_rt_graph_launch(void* exec);
void pa_rt_graph_free(void* exec);
void pa_rt_skip(int on);      /* 1: asynchronous device operations become no-ops (a graph queues them) */
int pa_rt_skipping(void);

/* ---- native RCCL hooks (comm_rccl.hip) --------------------------------- */
const char* pa_rccl_error(void);
int pa_rccl_available(void);
int pa_rccl_unique_id(char* id128);
int pa_rccl_init(const char* id128, int rank, int size);
void pa_rccl_shutdown(void);
int pa_rccl_allreduce(void* ctx, double* buf, int count);
int pa_rccl_exchange(void* ctx, const double* send, const int* send_counts, double* recv,
                     const int* recv_counts, const int* peers, int npeers);

/* ---- SpMM (utils/cplm_v0/cplm_v0_matmult_v2.c:108-343, K1) ------------- */
/* The local row panel in sliced-ELL form (SELL-64): rows are cut into slices
 * of 64 consecutive rows (slices never cross a subdomain), each slice padded to
 * its longest row and stored entry-major, so lane r of a wavefront reads
 * val[off + k*64 + r]: every load of the 12 B/nonzero stream is coalesced.
 * Padding entries carry value 0 and the row's own (diagonal) column. */
typedef struct {
  int m;                    /* local rows */
  int nslices;
  const long long* sl_off;  /* nslices+1: offset of the slice in val / col */
  const int* sl_len;        /* nslices: padded row length */
  const int* sl_row0;       /* nslices: first local row */
  const int* sl_nrows;      /* nslices: rows in the slice (<= 64) */
  const int* col;           /* local column: < m own row, >= m halo slot */
  const double* val;
  int nblk;                 /* workgroup blocks: consecutive slices of one subdomain */
  const int* blk_slice;     /* nblk+1: first slice of each block */
  const int* blk_win;       /* 2*nblk: [w0, w1) local X rows staged in LDS */
  const int* order;         /* block ids: interior blocks first, then blocks that read halo rows */
  int n_interior;
  int win_cap;              /* rows of the largest window */
  /* staged variant (preferred): every X row a block touches is copied to LDS
   * first -- its own row range, then the listed external rows -- and `col16`
   * holds the LDS slot of each entry (2 B per nonzero instead of 4). */
  int staged;
  const unsigned short* col16;
  const int* blk_ext_off;   /* nblk+1: range of the block in ext_rows */
  const int* ext_rows;      /* local row ids (>= m: halo slot) staged after the own rows */
  int stage_cap;            /* rows of the largest staging area */
  /* run variant of the staged plan: `col16` holds one LDS slot per run of three consecutive
   * slots and `val` three values per run ([k][3][lane], sl_off / sl_len count runs); the
   * staging area is [external rows below the own range | own rows | external rows above |
   * two zero rows], blk_nlow = how many of a block's external rows lie below its own range. */
  int runs;
  const int* blk_nlow;
  int runs_cols;            /* columns a workgroup of the run plan stages and computes (= the panel stride, or 8
                             * when a 16-column panel is split between two workgroups) */
  /* packed run plan (spmm_pack.h): `val` holds only the values that are not +0.0 and pk_meta four 64-bit words
   * per step -- three presence masks and the index of the step's part of `val`, a 0.0 and then its kept values;
   * sl_off / sl_len still count runs */
  int packed;
  const unsigned long long* pk_meta;
  /* non-NULL (packed run plan at up to 4 columns, preAlps_hip_set_operator_precision(32)): `val` rounded to fp32,
   * element for element (pa_k_plan_round_values), read through the same pk_meta in place of `val`; `val` stays */
  const float* val32;
  /* coded != 0 (packed run plan at 2 or 4 columns, spmm_code.h): `code` holds a 2-byte code per element of `val`,
   * read through the same pk_meta; code_tab[blk_tab_off[b] + c] is the value of code c in block b.  A block with an
   * empty table is read from `val`, which stays.  code_lds = LDS bytes of the block that needs most (staging rows,
   * zero rows, table). */
  int coded;
  const unsigned short* code;
  const double* code_tab;
  const int* blk_tab_off;
  int code_lds;
} pa_spmm_plan_t;
/* phase 0: interior blocks, 1: halo-reading blocks, 2: all.  exact != 0: read `val` even where val32 is set, and
 * leave every Gram request (pa_k_spmm_gram_arm) as it is. */
int pa_k_spmm(const pa_spmm_plan_t* pl, int ts, const double* X, const double* Xhalo,
              double* Y, int phase, int exact);
/* Ask the next product X -> Y of pa_k_spmm (4-column panels, run plan) to leave the partial
 * blocks of [Y | R]^T X (8 x 4 each, the layout of pa_k_gram with two panels) in `partials`
 * (room for cap blocks); pa_k_spmm_gram_take returns how many there are (0: the product ran
 * without them) and ends the request; pa_k_finish32 sums them (t > 0: and factors, as
 * pa_k_gram_finish does). */
void pa_k_spmm_gram_arm(const double* X, const double* Y, const double* R, double* partials, int cap);
void pa_k_spmm_gram_disarm(const double* owner);   /* owner: the request's partials (only that request ends); NULL: any */
long long pa_k_spmm_gram_launches(void);   /* launches of the SpMM with the Gram block so far */
int pa_k_spmm_gram_take(const double* X, const double* Y);
int pa_k_finish32(const double* partials, int nblk, double* scratch, int t, int T, double* out, double* mu,
                  double* alpha, int* info);       /* scratch: pa_finish32_scratch_blocks() x 32 doubles */
int pa_finish32_scratch_blocks(void);
/* Two pa_k_finish32 in one launch, each with its own partials, scratch and result, and the same sums as alone:
 * a (t > 0: factored, alpha formed, as pa_k_finish32) and b (summed only). */
int pa_k_finish32_pair(const double* pa, int na, double* sa, int t, int T, double* outa, double* mu, double* alpha,
                       int* info, const double* pb, int nb, double* sb, double* outb);
/* the same sum, followed by the residual norm from the update kernel's column sums (res2[0], res2[1] = *info) */
int pa_k_finish32_trace(const double* partials, int nblk, double* scratch, double* out, const double* rtr_partials,
                        int rtr_nblk, int ts, int nc, double* res2, int* info);
/* Ask the next block solve in -> out on a 4-column panel (every block through bj_g4.hip) to leave the partial
 * blocks of [in | prev]^T out behind, one per block; pa_k_bj_gram_take: how many there are (0: none). */
void pa_k_bj_gram_arm(const double* in, const double* out, const double* prev, double* partials, int cap);
void pa_k_bj_gram_disarm(const double* owner);
long long pa_k_bj_gram_applies(void);        /* block solves that left the Gram block behind so far */
int pa_k_bj_gram_take(const double* in, const double* out);
/* New values for the plan's value array (spmm_values.hip): val[s] = map[s] ? pv[map[s] - 1] : 0.0 for s < n, the
 * slots the upload copied (n even; entries past n are not touched).  map: spmm_plan.h, pa_spmm_plan_value_map;
 * pv: the panel's values in panel order.  All three on the device. */
int pa_k_plan_set_values(const unsigned* map, const double* pv, double* val, size_t n);
/* The same for a packed run plan (spmm_pack.h), over the n slots of the unpacked array: write = 0 counts into
 * *misses (device, zeroed by the caller) the slots whose new value is not +0.0 while the pack has no place for
 * it and writes nothing; write = 1 stores the new value of every slot that has a place in `packed`. */
int pa_k_pack_set_values(const unsigned* map, const double* pv, const unsigned long long* meta, double* packed,
                         size_t n, int write, unsigned* misses);
/* val32[i] = (float)val[i], i < n (spmm_values.hip: k_plan_round_values).  bad (device, two 8-byte words, zeroed by
 * the caller): bad[0] counts, as an integer, the values that are finite in fp64 and not in fp32; bad[1] receives the
 * bits of one of them. */
int pa_k_plan_round_values(const double* val, float* val32, size_t n, unsigned long long* bad);
/* sendbuf[i*ts + c] = X[idx[i]*ts + c] */
int pa_k_pack_rows(int n, int ts, const int* idx, const double* X, double* sendbuf);

/* HBM calibration: which = 0 copy src -> dst, 1 read src (dst receives nothing). */
int pa_k_probe(int which, size_t bytes, const double* src, double* dst);
int pa_k_spacer(int us);

/* ---- tall-skinny kernels (ecg.c:250,311,330,347,425,438,510 K2; K3; K4) -- */
/* Partial Gram blocks C = [A0 | A1]^T B over the local rows, one (npan*ts) x ts
 * column-major block per workgroup into `partials`; returns the number of
 * workgroups through nblk.  A1 may be NULL (npan = 1). */
int pa_k_gram(int m, int ts, const double* A0, const double* A1, const double* B,
              double* partials, int* nblk);
/* pa_k_gram + pa_k_finish.  With t > 0 (out = [W ; G^T], a_lo = nb = t, a_hi = T,
 * ld_out = t + T) the finishing launch goes on like pa_k_potrf_alpha on `out`. */
int pa_k_gram_finish(int m, int ts, const double* A0, const double* A1, const double* B,
                     double* partials, int a_lo, int a_hi, int nb, double* out, int ld_out, int t,
                     int T, double* mu, double* alpha, int* info);
/* pa_k_gram + one launch that sums the block (as pa_k_finish) and the residual norm (as
 * pa_k_trace_finish: res2[0] = norm^2, res2[1] = *info). */
int pa_k_gram_finish_trace(int m, int ts, const double* A0, const double* A1, const double* B, double* partials,
                           int a_lo, int a_hi, int nb, double* out, int ld_out, const double* rtr_partials,
                           int rtr_nblk, int nc, double* res2, const int* info);
int pa_gram_max_blocks(void);
/* out[i + ld_out*j] = sum over blocks, for rows i < a_lo (panel 0) and
 * a_lo <= i < a_lo + a_hi (panel 1, column i - a_lo), j < nb. */
int pa_k_finish(const double* partials, int nblk, int npan, int ts, int a_lo, int a_hi,
                int nb, double* out, int ld_out);
/* In-place upper Cholesky of the t x t column-major W (LAPACKE_dpotrf 'U',
 * ecg.c:318,431,577); *info (device int) = 0 or failing column + 1. */
int pa_k_potrf(double* W, int t, int* info);
/* The t x t part of one fused Orthodir step (ecg.c:577-587): Cholesky of mu,
 * beta <- beta U^-1, alpha <- U^-T alpha, beta(0:t,0:t) <- U^-T beta(0:t,0:t). */
int pa_k_fused_small(double* mu, int t, int nrhs, int bm, int bn, int ldb, double* alpha,
                     double* beta, int* info);
/* P <- P U^-1 and AP <- AP U^-1 on the first t columns (cblas_dtrsm Right,
 * Upper, ecg.c:324-327,434-435).  AP may be NULL. */
int pa_k_trsm(int m, int ts, int t, const double* U, double* P, double* AP);
/* X += P alpha, R -= AP alpha (ecg.c:337-338,500-501), alpha is t x nc with
 * leading dimension t; also the per-workgroup sums of R(:,c)^2 for the
 * stopping test (ecg.c:250) into rtr_partials[blk*ts + c]. */
int pa_k_update_xr(int m, int ts, int t, int nc, const double* alpha, const double* P,
                   const double* AP, double* X, double* R, double* rtr_partials, int* nblk,
                   int trace_nc, double* res2, const int* info, double* host);
/* trace_nc > 0: followed by pa_k_trace_finish over trace_nc columns into res2 and, when
 * `host` (pinned, device-visible) is given, into host[0..1] as well (no copy needed). */
/* buf = [W ; G^T] ((t+T) x t, leading dimension t+T) with W = AP^T P and G = P^T R of the
 * un-normalised P  ->  mu = chol(W) (upper, t x t), alpha = U^-T G (t x T, ld t). */
int pa_k_potrf_alpha(const double* buf, int t, int T, double* mu, double* alpha, int* info);
/* pa_k_trsm followed by pa_k_update_xr in one pass over P, AP, X, R.  gram != NULL: U and alpha
 * are outputs -- every workgroup computes them from gram = [W ; G^T] as pa_k_potrf_alpha does
 * (nc = T) and the first one stores them and *info. */
int pa_k_trsm_update(int m, int ts, int t, int nc, double* U, double* alpha, double* P,
                     double* AP, double* X, double* R, double* rtr_partials, int* nblk, int trace_nc,
                     double* res2, int* info, double* host, const double* gram, double* ukeep);
/* ukeep != NULL (lazy normalisation, panels of up to 4 columns): P and AP are NOT overwritten -- X and R get the
 * same update from rows normalised in registers -- and the t x t factor U is stored in ukeep for pa_k_update_z. */
/* pa_k_trsm_update (ukeep, no gram, no trace) and pa_k_update_z (ucur = U, uprev, V0 = P, V1 = P_prev, a_lo = a_hi =
 * nc = t) in one pass over P, AP, P_prev, X, R and Z: X += P U^-1 alpha, R -= AP U^-1 alpha, Z <- Z C0 - P C1 -
 * P_prev C2, U kept in ukeep, and the column sums of R^2 in pa_k_trsm_update's layout (*nblk blocks).  4-column
 * panels only. */
int pa_k_update_xrz(int m, int ts, int t, double* U, double* alpha, const double* P, const double* AP,
                    const double* P_prev, double* X, double* R, double* Z, double* rtr_partials, int* nblk,
                    double* ukeep, const double* beta, int ldb, const double* uprev);
/* The same pass with a choice of what happens to X (nobody reads X between two row passes of one call of the library's
 * loops).  xmode 0: pa_k_update_xrz.  1: X is neither read nor written -- the update is owed -- and alpha is kept in
 * akeep (t x t), as U is in ukeep.  2: the update owed by the pass before (P_prev, uprev and the alpha in akeep) and
 * then this one's, two additions to every x in that order: the bits of two passes of mode 0.  pa_k_flush_x: the owed
 * update alone, X += (P_prev uprev^-1) akeep, for a debt that no pass of mode 2 will pay. */
int pa_k_update_xrz_mode(int m, int ts, int t, double* U, double* alpha, const double* P, const double* AP,
                         const double* P_prev, double* X, double* R, double* Z, double* rtr_partials, int* nblk,
                         double* ukeep, const double* beta, int ldb, const double* uprev, int xmode, double* akeep);
int pa_k_flush_x(int m, int ts, int t, const double* uprev, const double* akeep, const double* P_prev, double* X);
/* Standalone sums of R(:,c)^2 (same layout as above). */
int pa_k_colnorm2(int m, int ts, const double* R, double* rtr_partials, int* nblk);
/* res2[0] = sum over blocks and columns c < nc; res2[1] = *info (0 if info is NULL). */
int pa_k_trace_finish(const double* rtr_partials, int nblk, int ts, int nc, double* res2,
                      const int* info, double* host);    /* host: pinned words that receive the same two values (may be NULL) */
/* Z(:, :nc) -= [V0(:, :a_lo) | V1(:, :a_hi)] beta, beta is (a_lo+a_hi) x nc,
 * leading dimension ldb (ecg.c:354,517). */
int pa_k_update_z(int m, int ts, int a_lo, int a_hi, int nc, const double* beta, int ldb,
                  const double* V0, const double* V1, double* Z, const double* note_src, double* note_host,
                  const double* ucur, const double* uprev, double* zz_part, int zz_cols, int* zz_nblk);
/* One-shot request to the next pa_k_update_z (panels of up to 4 columns): also copy the new row r of Z into the slots
 * pk_slot[pk_off[r] .. pk_off[r + 1]) of sendbuf (ts doubles each) -- the halo pack of the product that follows.
 * 0: not taken (wider panels; the caller must not tell the operator the rows are packed). */
int pa_k_update_z_pack(int ts, const int* pk_off, const int* pk_slot, double* sendbuf);
/* ucur != NULL (lazy normalisation): V0 / Z belong to the factor ucur, V1 to uprev, beta holds the raw Gram
 * blocks [V0-side ; V1-side]^T Z; the kernel applies U^-1 where the reference's panels would carry it. */
/* note_host != NULL: note_src[0..1] (device) are also written to note_host[0..1] (pinned, device-visible) */
/* The next launch that writes two words to pinned host memory (pa_k_trsm_update / pa_k_update_xr with
 * `host`, pa_k_update_z with note_host) also writes host[2] = seq behind them (seq != 0; one-shot), for
 * a host that polls that word instead of waiting for an event. */
void pa_k_note_seq(double seq);
/* Takes that number for a launch that writes to `host` (0 when host is NULL or none was set): the one copy of the
 * state, for the launchers of every kernel unit. */
double pa_k_take_note_seq(const double* host);
/* dst(:, :nc) = src(:, :nc) (mkl_domatcopy, ecg.c:358,521-523). */
int pa_k_copy_cols(int m, int ts, int nc, const double* src, double* dst);
/* A(:, :t) <- A(:, :t) Q, Q is t x t column-major (the effect of LAPACKE_dormqr
 * 'R','N' at ecg.c:476-479 with Q formed explicitly). */
int pa_k_right_mult(int m, int ts, int t, const double* Q, double* A);
/* A(:, j) <- A(:, piv[j]) for j < n (LAPACKE_dlapmt forward, ecg.c:380); piv 0-based, device. */
int pa_k_permute_trsm(int m, int ts, int n, const int* piv, int t, const double* U, const double* src, double* dst);
int pa_k_permute_cols(int m, int ts, int n, const int* piv, double* A);
/* sol[i] = sum_j X[i][j], j < nc (ecg.c:674). */
int pa_k_rowsum(int m, int ts, int nc, const double* X, double* sol);
/* Several right-hand sides: system j of k owns the columns j*s .. j*s + s - 1 (k*s <= ts).
 * R0 (m x ts, zero-filled) with B(row, j) in column j*s + pcol[row]; sums[blk*ts + j] = the block's share of
 * sum B(:, j)^2 (*nblk blocks, the layout of pa_k_colnorm2).  B: device, column major, ldb >= m; pcol: m ints. */
int pa_k_multi_start(int m, int ts, int k, int s, const double* B, int ldb, const int* pcol, double* R,
                     double* sums, int* nblk);
/* A start from an initial guess: X (m x ts) with X0(row, j) in column j*s + pcol[row], zero elsewhere.  X0: device,
 * column major, ld >= m. */
int pa_k_guess_split(int m, int ts, int k, int s, const double* X0, int ld, const int* pcol, double* X);
/* ... and R0 from AX = A X of that panel: B(row, j) - (the sum of the columns of system j of AX, ascending) in column
 * j*s + pcol[row], zero elsewhere.  bsums[blk*ts + j]: the block's share of sum B(:, j)^2, grid and order of
 * pa_k_multi_start; rsums[blk*ts + c]: its share of sum R0(:, c)^2, the layout of pa_k_colnorm2 (*nblk blocks each). */
int pa_k_guess_start(int m, int ts, int k, int s, const double* B, int ldb, const int* pcol, const double* AX,
                     double* R, double* bsums, double* rsums, int* nblk);
/* out[j] = sum over the columns of system j (ascending) of the sum over the blocks of rtr_partials[blk*ts + c],
 * one workgroup, fixed order; host (pinned, device-visible, may be NULL) receives the same k values. */
int pa_k_group_norms(const double* rtr_partials, int nblk, int ts, int k, int s, double* out, double* host);
/* The same k sums for a collective to carry (several processes): buf[2 + j] = the sum of system j, buf[0] = their sum
 * in ascending j (the local sum of squares of all of R), buf[1] = *info (NULL: 0); buf: 2 + k doubles on the device. */
int pa_k_group_norms_ride(const double* rtr_partials, int nblk, int ts, int k, int s, const int* info, double* buf);
/* sol[i + j*ld] = sum of X[i][c] over the columns of system j, ascending c (pa_k_rowsum per system). */
int pa_k_rowsum_groups(int m, int ts, int k, int s, const double* X, double* sol, int ld);
/* ---- the solution history (history.hip; preAlps_SolutionHistory*) ----
 * Xh: n x cap, column major (ldh), logical column i (0: the oldest) in slot (head + i) % cap; K <= cap live columns.
 * pa_k_hist_dots: out (K x q, ld K, device) = Xh^T W, W column major (ldw); pa_k_hist_dots_mapped: W is a panel of
 * the iteration (m rows of ts doubles) in the operator's internal space, Xh is read at row src[r] and W(r, :) divided
 * by dl[r].  part: pa_k_hist_part_doubles() doubles of scratch; the partial sums are folded in block order (no atomics:
 * two launches agree in bits).  pa_k_hist_combine: X0 (n x q, ldx0) = Xh c, c K x q (ld K) on the device, the oldest
 * column first.  K, q outside 1 .. 16, a ring that does not hold K, a leading dimension below n: refused. */
size_t pa_k_hist_part_doubles(void);
int pa_k_hist_dots(int n, int K, int q, const double* Xh, int ldh, int head, int cap, const double* W, int ldw,
                   double* part, double* out);
int pa_k_hist_dots_mapped(int m, int K, int q, const double* Xh, int ldh, int head, int cap, const int* src,
                          const double* dl, const double* Wp, int ts, double* part, double* out);
int pa_k_hist_combine(int n, int K, int q, const double* Xh, int ldh, int head, int cap, const double* c, double* X0,
                      int ldx0);
/* Several processes: the ring Xl holds the m rows this process owns (m x cap, ldh >= m); local row r is the caller's row
 * src[r] < N, and the caller's arrays (N rows, ld >= N) are touched at the owned rows alone.  part:
 * pa_k_hist_owned_part_doubles() doubles; red: the buffer one all-reduce carries (ecg_history.h: PA_HIST_RED_WORDS
 * doubles, the offsets from pa_hist_red_layout); a fold writes its two blocks and leaves word 0 and the rest alone.
 * pa_k_hist_gather: out(r, slots[j]) = a[src[r] + j lda] (slots on the host; NULL: column j to slot j; a negative slot
 * is skipped; every slot < cap).  pa_k_hist_ring_scaled: out(r, i) = Xl(r, i) / dl[r], i < K by physical slot.
 * pa_k_hist_project_owned: red[off_g ..) = Xl^T b[src] (K x q, ld K, logical order) and red[off_bb ..) = the q sums
 * b_j^2 over the owned rows, one launch and one fold; K = 0 is an empty ring.  pa_k_hist_gram_owned: W the panel (ts
 * doubles per row) divided by dl; red[off_do ..) = Xl^T W (K x q) and, with Xn (m x q in local row order, ldn),
 * red[off_dn ..) = Xn^T W (q x q).  pa_k_hist_combine_owned: X0[src[r] + j ldx0] = (Xl c)(r, j), the terms of
 * pa_k_hist_combine. */
size_t pa_k_hist_owned_part_doubles(void);
int pa_k_hist_gather(int m, int N, int q, const int* src, const double* a, int lda, const int* slots, int cap, double* out,
                     int ldo);
int pa_k_hist_ring_scaled(int m, int K, const double* Xl, int ldh, const double* dl, double* out, int ldo);
int pa_k_hist_project_owned(int m, int N, int K, int q, const double* Xl, int ldh, int head, int cap, const int* src,
                            const double* b, int ldb, double* part, double* red, int off_bb, int off_g);
int pa_k_hist_gram_owned(int m, int K, int q, const double* Xl, int ldh, int head, int cap, const double* Xn, int ldn,
                         const double* dl, const double* Wp, int ts, double* part, double* red, int off_do, int off_dn);
int pa_k_hist_combine_owned(int m, int N, int K, int q, const double* Xl, int ldh, int head, int cap, const double* c,
                            const int* src, double* X0, int ldx0);
/* ---- the caller's own system (dense_system.hip; preAlps_ECGSolveSystem) ----
 * Local row i is the caller's row src[i] with scaling factor dl[i] (1.0 when the operator is unscaled); src, dl: m
 * entries on the device.  B, X0, Xout: device, column major, k columns, rows in the caller's order, ld >= m.
 * Bp(i, j) = dl[i] * B(src[i], j) and, when X0 is given, X0p(i, j) = X0(src[i], j) / dl[i], both with leading dimension
 * m; sums[blk*ts + j] = the block's share of sum_i B(src[i], j)^2 (*nblk blocks, the layout of pa_k_colnorm2, for
 * pa_k_group_norms with s = 1).  B and X0 are only read. */
int pa_k_sys_gather(int m, int ts, int k, const int* src, const double* dl, const double* B, int ldb, const double* X0,
                    int ldx0, double* Bp, double* X0p, double* sums, int* nblk);
/* Xout(src[i], j) = dl[i] * (the sum of X[i][c] over the columns of system j, ascending c as pa_k_rowsum_groups). */
int pa_k_sys_scatter(int m, int ts, int k, int s, const double* X, const int* src, const double* dl, double* Xout,
                     int ldx);
/* part[blk*ts + j] = the block's share of sum_i ((sum of R[i][c] over the columns of system j, ascending) / dl[i])^2
 * (*nblk blocks): ||b_j - A x_j||^2 in the caller's units once pa_k_group_norms with s = 1 has folded them. */
int pa_k_sys_norms(int m, int ts, int k, int s, const double* R, const double* dl, double* part, int* nblk);
/* Xout(src[i], j) = Xin(src[i], j) for the m rows of the map and k columns (device arrays, the caller's order). */
int pa_k_sys_copy_rows(int m, int k, const int* src, const double* Xin, int ldin, double* Xout, int ldout);
/* The caller's metric on several processes, for a collective to carry: buf[0] = the local scaled sum of squares of all of
 * R, folded from rtr_part (rtr_nblk blocks of column sums) as pa_k_group_norms_ride folds it -- the same bits --,
 * buf[1] = *info (NULL: 0), buf[2 + j] = the fold of sys_part (sys_nblk blocks, what pa_k_sys_norms left) for system j;
 * buf: 2 + k doubles on the device, nothing else is written.  Refuses k * s > ts and a NULL buf. */
int pa_k_sys_norms_ride(const double* rtr_part, int rtr_nblk, const double* sys_part, int sys_nblk, int ts, int k, int s,
                        const int* info, double* buf);
/* ---- the energy-norm drops of an iteration (dense_energy.hip; preAlps_ECGSolveSystemEnergy) ----
 * alpha: rows x T on the device, column major with leading dimension ld, the coefficients of A-orthonormal directions
 * that the update of X uses; system j of k owns its columns j*s .. j*s + s - 1.  out[j] = sum_r (sum_{c in G_j}
 * alpha(r, c))^2, the inner sums in ascending c, the outer in ascending r (one fma each); host (pinned,
 * device-visible, may be NULL) receives the same k values.  One workgroup, no atomics: two launches agree in bits.
 * Refuses a NULL alpha or out, rows or T outside 1 .. 16, ld < rows, k < 1, s < 1 and k * s > T. */
int pa_k_energy_drops(const double* alpha, int rows, int ld, int T, int k, int s, double* out, double* host);

/* ---- block-Jacobi apply (block_jacobi.c:93-109, K8) --------------------- */
/* the pair tasks of one class: device array of (i0, i1), positions into the class's list (i1 = -1: no partner) */
typedef struct { const int* tasks; int ntasks, paired; } pa_bj_ptask_t;
typedef struct {
  int nparts;              /* blocks owned by this process */
  const int* row0;         /* nparts: first local row of each block */
  const int* nrows;        /* nparts */
  const int* bw;           /* nparts: bandwidth w of the block's factor */
  const long long* off;    /* nparts: offset (doubles, even) of the block in Lf / Lb */
  const int* map_f;        /* local row visited at forward step j (m entries) */
  const int* map_b;        /* local row visited at backward step j */
  /* Narrow bands: one record of wr = (w+1 rounded up to even) doubles per step:
   * forward  Lf[off + j*wr + d-1] = L(j+d, j) / L(j,j),                 d = 1..w, then a zero
   * backward Lb[off + j*wr + d-1] = L(b-1-j, b-1-j-d) / L(b-1-j, b-1-j).
   * Wide bands: records of W = pa_bj_wide_window(w) doubles, the value for target row i at i mod W.
   * Arrays are padded by 2 KiB at the end. */
  const double* Lf;
  const double* Lb;
  /* optional (NULL: absent): the same records in pairs for the classes R = 2, 3 (k_bj_pairs), block p at
   * off2[p]: per chunk of 8 steps two sub-blocks of [2 pivot pairs][w + 4 target rows] double2 */
  const double* Lf2; const double* Lb2; const long long* off2;
  /* optional (NULL: absent): ONE copy of the factor for both sweeps of panels of up to 4 columns, in
   * selective-inversion form by groups of four pivots (bj_g4.hip), block p at off2[p]: per group
   * (w + 4) rows x 4 pivots of M = [T - I ; -G], eligible classes flagged in class_g4 */
  const void* Lg4;        /* records of g4_bits bits: double, or float (PREALPS_BJ_BAND_PRECISION=single); off2 counts elements */
  int g4_bits;            /* 64 / 32; 0 when Lg4 is absent */
  const int* class_g4;    /* host array, nclass: 1 = every block of the class has a record in Lg4 */
  const int* class_bmax;   /* host array, nclass: most rows of a block in the class */
  const double* invd_f;    /* 1 / L(j,j) in forward step order (m entries) */
  const double* invd_b;    /* ... in backward step order */
  int nclass;              /* parts grouped by register sets R = ceil((w+64)/64) of the one-wavefront kernel */
  const int* class_R;      /* host array, nclass: register sets per lane; < 0: wide class (workgroup per block) */
  const int* class_count;  /* host array */
  const int* class_wmax;   /* host array: widest band in the class (sizes the LDS chunks) */
  const int* const* class_list; /* host array of device pointers to part ids */
  /* optional (NULL: absent): the pair tasks of the classes that bj_g4.hip serves from fp64 records (bj_share.h:
   * pa_bj_pair_tasks), two blocks of one class of identical blocks per wavefront */
  const pa_bj_ptask_t* class_ptask;  /* host array, nclass */
  int pair_mode;           /* PREALPS_BJ_PAIR: 0 never, 1 whenever a list has a pair, -1 (absent) the rule of bj_g4_plan.c */
  int pair_intact;         /* 1: every block reads the records it read at the create (no refresh has split a class) */
} pa_bj_plan_t;
/* Window of a wide block (rows in flight = record length, >= w + 64) for bandwidth w: a multiple of the
 * 64 / 128 / 256 rows that 1 / 2 / 4 register sets per lane hold across a wavefront.  The one rule for the
 * host layout (block_jacobi.c) and the kernels (bj_band.hip). */
#ifdef __HIPCC__
#define PA_HOST_DEVICE __host__ __device__
#else
#define PA_HOST_DEVICE
#endif
static inline PA_HOST_DEVICE int pa_bj_wide_window(int w) {
  int W = (w + 64 + 63) & ~63;
  if (W <= 1024) return W;
  W = (w + 64 + 127) & ~127;
  if (W <= 2048) return W;
  return (w + 64 + 255) & ~255;
}
/* pt: the pair tasks of `list` (NULL: none); whether the launch pairs is decided by the planner (bj_g4_plan.c: the
 * rule).  A launch the planner refuses returns 1 with the reason in pa_rt_error(). */
int pa_k_bj_g4(const pa_bj_plan_t* pl, const int* list, int count, int wmax, int bmax, int xs, int ncol,
                const double* in, double* out, const pa_bj_ptask_t* pt);
/* One-shot: the next pa_k_bj_g4 on a 4-column panel also leaves the 8 x 4 block [in | prev]^T out of every
 * block in part (32 doubles per block, in the order of its list; the layout of pa_k_gram with two panels). */
void pa_k_bj_g4_gram(const double* prev, double* part);
int pa_k_bj_pairs(const int* list, int count, const int* nrows, const int* bw, const long long* off,
                  const long long* off2, const double* L, double* L2);
/* bj_g4.hip: the records of Lg4 from the plain forward records, and the block solve that reads them
 * (blocks of at most pa_bj_g4_max_rows() rows, bands up to pa_bj_g4_max_band(): bj_g4_plan.h, which knows the
 * limits); `in` / `out` point at the first of up to four columns of panels with row stride xs. */
int pa_k_bj_g4_setup(const int* list, int count, const int* nrows, const int* bw, const long long* off,
                      const long long* off2, const double* L, double* Lg4);
/* the same records rounded to fp32: (float)v of the same fp64 value at the same position */
int pa_k_bj_g4_setup_f32(const int* list, int count, const int* nrows, const int* bw, const long long* off,
                          const long long* off2, const double* L, float* Lg4);
/* the last launch of pa_k_bj_g4: 0 = ring depth, 1 = storage bits of the records it read, 2 = 1 if it was the
 * pipelined few-blocks chain, 3 = 1 if it was the PAIR launch (two blocks of one class per wavefront) */
int pa_bj_g4_last(int which);
/* dst[off[e]] = val[e], e < n */
int pa_k_scatter(size_t n, const long long* off, const double* val, double* dst);
/* Wider bands (up to 4032): `band` diagonal-major per block (A(i, i-d) at boff + d*nrows + i),
 * factored in place (blocked, one workgroup per block), then laid out into Lf / Lb / invd
 * (records in window-slot order for bands above wide_from, else [d = 1..w | 0]). */
int pa_k_bj_factor_big(const int* list, int count, int wmax, int wide_from, const int* row0, const int* nrows,
                       const int* bw, const long long* off, const long long* boff, double* band, double* Lf, double* Lb,
                       double* invd_f, double* invd_b, int* fail);
/* Band Cholesky on the device for blocks with bandwidth <= pa_bj_factor_wmax(): `band` holds
 * each listed block's rows in factor order, (w+1) doubles per row (A(i, i-d) at d), at offset
 * boff[part]; writes the forward / backward sweep records and 1/L(j,j) straight into Lf, Lb
 * (pre-zeroed), invd_f, invd_b.  *fail (device, pre-zeroed) = 1 + local position of the first
 * non-positive pivot seen. */
int pa_k_bj_factor(const int* list, int count, int wmax, const int* row0, const int* nrows, const int* bw,
                   const long long* off, const long long* boff, const double* band, double* Lf, double* Lb,
                   double* invd_f, double* invd_b, int* fail);
/* the block solve out = M^-1 in on panels of row stride ts: every class through the family bj_band_plan.c picks for it */
int pa_k_bj_apply(const pa_bj_plan_t* pl, int ts, const double* in, double* out);
/* bj_refactor.hip: band[boff[chunk_blk[c]] + dst[e]] = pv[src[e]] for the entries e of every chunk c of the band
 * map (bj_band_map.h); band zeroed beforehand, everything on the device. */
int pa_k_bj_band_assemble(const unsigned* src, const unsigned* dst, const int* chunk_blk, const unsigned* chunk_first,
                          size_t nchunks, const long long* boff, const double* pv, double* band);
/* bj_refactor.hip: for the `count` blocks p of `list`, off_read[p] / off2_read[p] = off / off2 of rep[p] if the assembled
 * bands of p and rep[p] are the same 64-bit words, of p itself if not; cnt[0] += blocks that still share, cnt[1] += the
 * elements of their second records (cnt zeroed by the caller; off2 / off2_read may be null) */
int pa_k_bj_share_check(const int* list, int count, const int* rep, const int* nrows, const int* bw, const long long* boff,
                        const double* band, const long long* off, const long long* off2, long long* off_read,
                        long long* off2_read, unsigned long long* cnt);

/* ---- coarse correction of the two-level block-Jacobi preconditioner (coarse.hip) -------------------------
 * out(:, :ncols) += Z Einv Z^T in(:, :ncols), every array on the device, fp64.  Z as zv (m x k row major: row i of
 * a chunk of aggregate g has its k values in the columns g*k .. g*k + k - 1 of Z), the chunk lists and Einv
 * (nc x nc, nc = naggr * k) as coarse_space.h lays them out.  Three stages on the library stream, no atomics (an
 * apply is reproducible in bits): k_coarse_restrict, one workgroup per chunk, partial[chunk][a][c] = sum_i zv[i][a]
 * in[i][c]; k_coarse_gather + k_coarse_einv, c[g*k + a][:] = the sum of aggregate g's chunk partials in list
 * order and y = Einv c in one pass over Einv; k_coarse_prolong_add, out[i][c] += sum_a zv[i][a] y[g(i)*k + a][c].
 * partial: nchunks * k * 16 doubles, c and y: nc * 16 doubles (scratch the plan owns).
 *   Several processes (rows != NULL): zv and the chunk lists are those of the rank's rows, agg_ptr lists all naggr
 * aggregates (empty where the rank has no chunk, so the gather leaves zeros there), and Einv holds only the nrows rows
 * of the inverse named in `rows` (ascending; the rows of the aggregates with a chunk here), nrows x nc row major.
 * The apply is restrict, gather, pa_allreduce(c, nc * ts), k_coarse_einv_rows (y[rows[x]] = Einv[x] . c, the other
 * rows of y are neither written nor read), prolong: one all-reduce more than on one process, on the library stream. */
typedef struct {
  int m, k, naggr, nc, nchunks;
  const double* zv;
  const int* ch_row0; const int* ch_nrows; const int* ch_aggr;
  const int* agg_ptr; const int* agg_chunk;
  const double* Einv;
  double* partial; double* c; double* y;
  int nrows; const int* rows;
} pa_coarse_plan_t;
int pa_k_coarse_apply(const pa_coarse_plan_t* pl, int ts, int ncols, const double* in, double* out);
/* y[rows[x]][:] = slab[x][:] . c for x < nrows (slab: nrows x nc row major, c and y: nc rows of ts doubles, rows: nrows
 * distinct ids in [0, nc)); one fixed order of additions per row, no atomics.  ts: 2, 4, 8 or 16. */
int pa_k_coarse_einv_rows(int nc, int nrows, const int* rows, const double* slab, const double* c, double* y, int ts);

/* ---- sparse block solve for large diagonal blocks (nd.c) --------------------------------- */
/* Supernodes of a nested-dissection Cholesky factor, all blocks of the process in one numbering.
 * Supernode s: n[s] pivot columns, m[s] rows below, panel P = [T ; -G] (see nd_apply.hip) twice:
 * F + offF[s] column major with leading dimension ld[s] >= n + m, B + offB[s] row major with row
 * length PA_ND_LD(n); only the entries below the diagonal are read.  rows[rows_off[s] + r] =
 * local panel row of front row r; src[2 (rows_off[s] + r) + c] = where front row r finds the
 * contribution of child c (row of its vector, -1: none), that vector starting at row
 * ccoff[2 s + c] of `contrib`; this supernode's own contribution starts at row coff[s].
 * dinv[local row] = 1 / L(row, row).  Y: scratch panel for the forward result (local rows).
 * Kernels: nd_apply.hip. */
/* leading dimensions of both copies: multiples of 128 bytes, so that the 512-byte segment a
 * wavefront loads never straddles an extra cache line */
#define PA_ND_LD(x) (((x) + 15) & ~15)
typedef struct {
  const int* n; const int* m; const int* ld; const long long* offF; const long long* offB; const int* rows_off;
  const int* coff; const int* ccoff; const int* rows; const int* src; const double* dinv;
  const double* F; const double* B; double* contrib; double* Y;
  const float* F32; const float* B32;   /* non-NULL: the same two copies rounded to fp32 (F / B released), read instead */
  int nlevel;                  /* levels of the forest, bottom-up; host arrays of device pointers: */
  const int* f_count; const int* const* f_front; const int* const* f_row0;   /* forward: (front, first front row) per workgroup */
  const int* b_count; const int* const* b_front; const int* const* b_col0;   /* backward: (front, first pivot column) per workgroup */
} pa_nd_plan_t;
/* ---- numeric factorisation of those blocks on the device (nd_factor.hip) ------------------- */
/* n, m, ld, offF, offB, rows_off, rows, src, F, B, dinv as in pa_nd_plan_t.  front[s] = device
 * address of the dense front of supernode s while its level (and its parent's) is being worked on:
 * column major, leading dimension ld[s], lower triangle.  child[2 s + c] = supernode id of child c
 * (-1: none); newrow[rows_off[s] + r] = index of front row r in its block's elimination order;
 * the block's own entries of the pivot columns of s: columns acp[acol0[s] + j] .. of (ari, acv),
 * rows in elimination order, lower triangle.  fail: smallest (supernode << 32 | pivot column) whose
 * pivot was not positive, ~0 if none; fail[1]: see pa_k_ndf_check. */
typedef struct {
  const int* n; const int* m; const int* ld; const long long* offF; const long long* offB; const int* rows_off;
  const int* rows; const int* src; const int* child; const int* newrow;
  const long long* acol0; const long long* acp; const int* ari; const double* acv;
  const unsigned long long* front; const int* ldf;
  double* F; double* B; double* dinv; unsigned long long* fail;
} pa_ndf_args_t;
/* tiles = (front, tile row, tile column) of 64 x 64 entries; chunks = (front, first row) of
 * pa_nd_chunk_rows() rows; jb = first pivot of the step (a multiple of 64) */
int pa_k_ndf_assemble(const pa_ndf_args_t* a, const int* tf, const int* ti, const int* tj, int ntiles,
                      const int* fronts, int nfronts);
int pa_k_ndf_potrf(const pa_ndf_args_t* a, const int* fronts, int nfronts, int jb);
int pa_k_ndf_trsm(const pa_ndf_args_t* a, const int* cfront, const int* crow0, int nchunks, int jb, int inverse);
int pa_k_ndf_update(const pa_ndf_args_t* a, const int* tf, const int* ti, const int* tj, int ntiles, int jb,
                    int inverse);
int pa_k_ndf_pinit(const pa_ndf_args_t* a, const int* cfront, const int* crow0, int nchunks);
int pa_k_ndf_finalize(const pa_ndf_args_t* a, const int* tf, const int* ti, const int* tj, int ntiles);
/* after finalize: fail[1] = max over the fronts of |L_11 (L_11^-1 1) - 1| with the inverse taken from the
 * finished panels (bit pattern of a non-negative double) */
int pa_k_ndf_check(const pa_ndf_args_t* a, const int* fronts, int nfronts, int nmax);

int pa_nd_chunk_rows(void);           /* front rows per forward workgroup */
int pa_nd_block_cols(void);           /* pivot columns per backward workgroup */
int pa_k_nd_apply(const pa_nd_plan_t* pl, int ts, const double* in, double* out);
/* dst[i] = src[i] rounded to the nearest float, i < n (nd_apply.hip) */
int pa_k_nd_round(const double* src, float* dst, size_t n);

#ifdef __cplusplus
}
#endif
#endif
