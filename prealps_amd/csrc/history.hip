// history.hip -- the device side of the solution history (preAlps_SolutionHistory*, solution_history.c): the dots of the ring
// of stored solutions with a block of columns, and the combination x0 = Xh c.  Written for gfx950 (wave64).
//   Xh: N x cap doubles, column major with leading dimension ldh, in the caller's order and units.  Logical column i
// (0: the oldest) lies in slot (head + i) % cap (ecg_history.h).
//   k_hist_dots leaves per workgroup the partial sums of Xh(:, i)^T W(:, j), i < K, j < q, in part[blk*256 + i + 16 j];
// k_hist_fold adds the workgroups' partials in ascending block order, one thread per entry: no atomics, and the
// result depends on N, K, q alone, so two launches agree in bits.  The q columns are taken four at a time (blockIdx.y):
// 16 x 4 accumulators per lane instead of 16 x 16, at the price of reading Xh once per four columns of W.
//   The plain form reads W column major (ldw).  The mapped form takes W as a panel of the iteration (row major, ts
// doubles per row) in the operator's internal space -- local row r is the caller's row src[r], scaled by dl[r] -- and
// forms Xh(src[r], i) * (W(r, j) / dl[r]): with W = A' x' that is Xh^T (A x) in the caller's units.
//   Both stream (K ceil(q / 4) + q) N doubles; k_hist_combine streams (K + q) N.
//   Several processes: the ring holds the rows a process owns, and a second family of kernels ("owned rows" below) reads
// and writes the caller's global arrays through the row map; their sums land in the buffer one all-reduce carries.  The
// kernels above and their launchers serve one process and are not touched by that family.
#include "kernels_common.h"

namespace {

constexpr int HIST_MAX = 16;
constexpr int HIST_QT = 4;               // columns of W per workgroup
constexpr int HIST_MAX_BLOCKS = 256;     // row blocks: the fold reads that many partials per entry
constexpr int HIST_PART = HIST_MAX * HIST_MAX;

// logical column i of a ring whose oldest column lies in slot head (head < cap, i < cap): wave-uniform
__device__ __forceinline__ int ring_slot(int head, int i, int cap) { const int s = head + i; return s >= cap ? s - cap : s; }

template <bool MAPPED>
__global__ __launch_bounds__(WG, 2) void k_hist_dots(size_t n, int K, int q, const double* __restrict__ Xh, size_t ldh,
                                                  int head, int cap, const int* __restrict__ src,
                                                  const double* __restrict__ dl, const double* __restrict__ W,
                                                  size_t ldw, double* __restrict__ part) {
  __shared__ double red[WG / 64][HIST_MAX * HIST_QT];
  const int j0 = blockIdx.y * HIST_QT;
  double acc[HIST_MAX][HIST_QT];
#pragma unroll
  for (int i = 0; i < HIST_MAX; ++i)
#pragma unroll
    for (int t = 0; t < HIST_QT; ++t) acc[i][t] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
#pragma unroll 1
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < n; row += stride) {
    double w[HIST_QT];
    size_t xrow = row;
    if (MAPPED) {
      xrow = (size_t)src[row];
      const double d = dl[row];
#pragma unroll
      for (int t = 0; t < HIST_QT; ++t) w[t] = (j0 + t < q) ? W[row * ldw + (size_t)(j0 + t)] / d : 0.0;
    } else {
#pragma unroll
      for (int t = 0; t < HIST_QT; ++t) w[t] = (j0 + t < q) ? W[row + (size_t)(j0 + t) * ldw] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < HIST_MAX; ++i)
      if (i < K) {
        const double x = Xh[xrow + (size_t)ring_slot(head, i, cap) * ldh];
#pragma unroll
        for (int t = 0; t < HIST_QT; ++t) acc[i][t] = fma(x, w[t], acc[i][t]);
      }
  }
  // the wavefront's 64 sums in 63 exchanges: at distance o a lane keeps the half of its values whose index has the
  // lane's bit o and hands the other half over, so lane l ends with the whole sum of entry l = i * 4 + t; then the
  // four wavefronts' through LDS in ascending order
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double a[HIST_MAX * HIST_QT];
#pragma unroll
  for (int i = 0; i < HIST_MAX; ++i)
#pragma unroll
    for (int t = 0; t < HIST_QT; ++t) a[i * HIST_QT + t] = acc[i][t];
#pragma unroll
  for (int half = 32; half >= 1; half >>= 1) {
    const bool up = (lane & half) != 0;
#pragma unroll
    for (int k = 0; k < half; ++k) {
      const double keep = up ? a[k + half] : a[k];
      const double send = up ? a[k] : a[k + half];
      a[k] = keep + __shfl_xor(send, half);
    }
  }
  red[wave][lane] = a[0];
  __syncthreads();
  if (threadIdx.x < HIST_MAX * HIST_QT) {
    const int i = threadIdx.x / HIST_QT, t = threadIdx.x % HIST_QT;
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < WG / 64; ++wv) s += red[wv][threadIdx.x];
    if (i < K && j0 + t < q) part[(size_t)blockIdx.x * HIST_PART + i + HIST_MAX * (j0 + t)] = s;
  }
}

// out(i, j) (K x q, ld K) = the partials of entry (i, j) added in ascending block order; one workgroup of 256
__global__ __launch_bounds__(HIST_PART) void k_hist_fold(int nblk, int K, int q, const double* __restrict__ part,
                                                         double* __restrict__ out) {
  const int i = threadIdx.x % HIST_MAX, j = threadIdx.x / HIST_MAX;
  if (i >= K || j >= q) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(size_t)b * HIST_PART + threadIdx.x];
  out[i + K * j] = s;
}

// X0(r, j) = sum_i Xh(r, slot(i)) c(i, j), i ascending (the oldest column first), one fma per term; c: K x q, ld K
__global__ __launch_bounds__(WG) void k_hist_combine(size_t n, int K, int q, const double* __restrict__ Xh, size_t ldh,
                                                     int head, int cap, const double* __restrict__ c,
                                                     double* __restrict__ X0, size_t ldx0) {
  __shared__ double cs[HIST_PART];
  for (int e = threadIdx.x; e < K * q; e += WG) cs[e] = c[e];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < n; row += stride) {
    double x[HIST_MAX];
#pragma unroll
    for (int i = 0; i < HIST_MAX; ++i) x[i] = i < K ? Xh[row + (size_t)ring_slot(head, i, cap) * ldh] : 0.0;
    for (int j = 0; j < q; ++j) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < HIST_MAX; ++i)
        if (i < K) s = fma(x[i], cs[i + K * j], s);
      X0[row + (size_t)j * ldx0] = s;
    }
  }
}

// ---- several processes: the ring holds the rows this process owns ----------------------------------------------------
// Xl: m x cap, column major with leading dimension ldh; local row r is the caller's row src[r], in the caller's units.
// The caller's arrays (b, x, x0: N rows) are read and written through src at the owned rows and nowhere else.  The
// partial sums of one launch lie in two regions of HIST_MAX_BLOCKS * 256 doubles each; k_hist_fold_red folds both in
// ascending block order and writes the entries behind word 0 of the buffer one all-reduce carries (ecg_history.h:
// pa_hist_red_layout gives the offsets).
constexpr int HIST_REGION = HIST_MAX_BLOCKS * HIST_PART;
constexpr int HIST_RED_WORDS = 1 + 16 + 256 + 256;

struct hist_slots_t { int s[HIST_MAX]; };

// out(r, slot[j]) = a[src[r] + j lda], j < q; a column whose slot is negative is not kept
__global__ __launch_bounds__(WG) void k_hist_gather(size_t m, int q, const int* __restrict__ src,
                                                    const double* __restrict__ a, size_t lda, hist_slots_t slots,
                                                    double* __restrict__ out, size_t ldo) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < m; row += stride) {
    const size_t from = (size_t)src[row];
#pragma unroll
    for (int j = 0; j < HIST_MAX; ++j)
      if (j < q && slots.s[j] >= 0) out[row + (size_t)slots.s[j] * ldo] = a[from + (size_t)j * lda];
  }
}

// out(r, i) = Xl(r, i) / dl[r], i < K by physical slot: the ring in the operator's units, as k_sys_gather leaves a guess
__global__ __launch_bounds__(WG) void k_hist_ring_scaled(size_t m, int K, const double* __restrict__ Xl, size_t ldh,
                                                         const double* __restrict__ dl, double* __restrict__ out,
                                                         size_t ldo) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < m; row += stride) {
    const double d = dl[row];
#pragma unroll
    for (int i = 0; i < HIST_MAX; ++i)
      if (i < K) out[row + (size_t)i * ldo] = Xl[row + (size_t)i * ldh] / d;
  }
}

// The dots of owned rows.  PANEL = false, the projection: W(r, j) = b[src[r] + j ldw] read straight from the caller's
// array, left operand the ring in logical order (head, cap); region 0 receives Xl^T b, region 1 the sums b_j^2 at entry
// 16 j.  PANEL = true, the Gram blocks: W(r, j) = Wp[r ts + j] / dl[r]; blockIdx.z = 0: left operand the ring (KL = K
// columns, head, cap) into region 0, blockIdx.z = 1: the q new columns Xn in local row order (ld ldn) into region 1.
template <bool PANEL>
__global__ __launch_bounds__(WG, 2) void k_hist_dots_owned(size_t m, int K, int q, const double* __restrict__ Xl, size_t ldh,
                                                        int head, int cap, const double* __restrict__ Xn, size_t ldn,
                                                        const int* __restrict__ src, const double* __restrict__ dl,
                                                        const double* __restrict__ W, size_t ldw,
                                                        double* __restrict__ part) {
  __shared__ double red[WG / 64][HIST_MAX * HIST_QT];
  __shared__ double red2[WG / 64][HIST_QT];
  const int j0 = blockIdx.y * HIST_QT;
  const bool fresh = PANEL && blockIdx.z == 1;          // workgroup-uniform
  const double* __restrict__ L = fresh ? Xn : Xl;
  const size_t ldl = fresh ? ldn : ldh;
  const int KL = fresh ? q : K, hd = fresh ? 0 : head, cp = fresh ? q : cap;
  double acc[HIST_MAX][HIST_QT], sq[HIST_QT];
#pragma unroll
  for (int i = 0; i < HIST_MAX; ++i)
#pragma unroll
    for (int t = 0; t < HIST_QT; ++t) acc[i][t] = 0.0;
#pragma unroll
  for (int t = 0; t < HIST_QT; ++t) sq[t] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
#pragma unroll 1
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < m; row += stride) {
    double w[HIST_QT];
    if (PANEL) {
      const double d = dl[row];
#pragma unroll
      for (int t = 0; t < HIST_QT; ++t) w[t] = (j0 + t < q) ? W[row * ldw + (size_t)(j0 + t)] / d : 0.0;
    } else {
      const size_t from = (size_t)src[row];
#pragma unroll
      for (int t = 0; t < HIST_QT; ++t) {
        w[t] = (j0 + t < q) ? W[from + (size_t)(j0 + t) * ldw] : 0.0;
        sq[t] = fma(w[t], w[t], sq[t]);
      }
    }
#pragma unroll
    for (int i = 0; i < HIST_MAX; ++i)
      if (i < KL) {
        const double x = L[row + (size_t)ring_slot(hd, i, cp) * ldl];
#pragma unroll
        for (int t = 0; t < HIST_QT; ++t) acc[i][t] = fma(x, w[t], acc[i][t]);
      }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double a[HIST_MAX * HIST_QT];
#pragma unroll
  for (int i = 0; i < HIST_MAX; ++i)
#pragma unroll
    for (int t = 0; t < HIST_QT; ++t) a[i * HIST_QT + t] = acc[i][t];
  // (the exchange of k_hist_dots: lane l ends with the whole sum of entry l = i * 4 + t)
#pragma unroll
  for (int half = 32; half >= 1; half >>= 1) {
    const bool up = (lane & half) != 0;
#pragma unroll
    for (int k = 0; k < half; ++k) {
      const double keep = up ? a[k + half] : a[k];
      const double send = up ? a[k] : a[k + half];
      a[k] = keep + __shfl_xor(send, half);
    }
  }
  red[wave][lane] = a[0];
  if (!PANEL) {
#pragma unroll
    for (int t = 0; t < HIST_QT; ++t) {
      double v = sq[t];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0) red2[wave][t] = v;
    }
  }
  __syncthreads();
  double* __restrict__ mine = part + (fresh ? (size_t)HIST_REGION : 0) + (size_t)blockIdx.x * HIST_PART;
  if (threadIdx.x < HIST_MAX * HIST_QT) {
    const int i = threadIdx.x / HIST_QT, t = threadIdx.x % HIST_QT;
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < WG / 64; ++wv) s += red[wv][threadIdx.x];
    if (i < KL && j0 + t < q) mine[i + HIST_MAX * (j0 + t)] = s;
  } else if (!PANEL && threadIdx.x < HIST_MAX * HIST_QT + HIST_QT) {
    const int t = threadIdx.x - HIST_MAX * HIST_QT;
    double s = red2[0][t];
#pragma unroll
    for (int wv = 1; wv < WG / 64; ++wv) s += red2[wv][t];
    if (j0 + t < q) part[(size_t)HIST_REGION + (size_t)blockIdx.x * HIST_PART + HIST_MAX * (j0 + t)] = s;
  }
}

// red[off + i + rows j] = the partials of entry (i, j) of a region added in ascending block order, for two blocks at
// once: threads 0 .. 255 the block a, 256 .. 511 the block b.  Word 0 and every word outside the two blocks stay.
struct hist_block_t { int region, rows, cols, off; };
__global__ __launch_bounds__(2 * HIST_PART) void k_hist_fold_red(int nblk, const double* __restrict__ part, hist_block_t a,
                                                                 hist_block_t b, double* __restrict__ red) {
  const hist_block_t blk = threadIdx.x < HIST_PART ? a : b;
  const int e = threadIdx.x % HIST_PART, i = e % HIST_MAX, j = e / HIST_MAX;
  if (i >= blk.rows || j >= blk.cols) return;
  const double* __restrict__ p = part + (size_t)blk.region * HIST_REGION;
  double s = 0.0;
  for (int bk = 0; bk < nblk; ++bk) s += p[(size_t)bk * HIST_PART + e];
  red[blk.off + i + blk.rows * j] = s;
}

// X0(src[r], j) = sum_i Xl(r, slot(i)) c(i, j), the terms and their order those of k_hist_combine; a row this process
// does not own is not written
__global__ __launch_bounds__(WG) void k_hist_combine_owned(size_t m, int K, int q, const double* __restrict__ Xl, size_t ldh,
                                                           int head, int cap, const double* __restrict__ c,
                                                           const int* __restrict__ src, double* __restrict__ X0,
                                                           size_t ldx0) {
  __shared__ double cs[HIST_PART];
  for (int e = threadIdx.x; e < K * q; e += WG) cs[e] = c[e];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < m; row += stride) {
    double x[HIST_MAX];
#pragma unroll
    for (int i = 0; i < HIST_MAX; ++i) x[i] = i < K ? Xl[row + (size_t)ring_slot(head, i, cap) * ldh] : 0.0;
    const size_t to = (size_t)src[row];
    for (int j = 0; j < q; ++j) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < HIST_MAX; ++i)
        if (i < K) s = fma(x[i], cs[i + K * j], s);
      X0[to + (size_t)j * ldx0] = s;
    }
  }
}

inline int hist_blocks(int n) {
  long long b = ((long long)n + 4LL * WG - 1) / (4LL * WG);
  if (b < 1) b = 1;
  return (int)(b < HIST_MAX_BLOCKS ? b : HIST_MAX_BLOCKS);
}

inline int combine_blocks(int n) {
  long long b = ((long long)n + WG - 1) / WG;
  if (b < 1) b = 1;
  return (int)(b < 2048 ? b : 2048);
}

inline int hist_args_bad(const char* what, int n, int K, int q, int ldh, int head, int cap) {
  if (n >= 0 && K >= 1 && K <= HIST_MAX && q >= 1 && q <= HIST_MAX && cap >= K && cap <= HIST_MAX && head >= 0 &&
      head < cap && ldh >= n)
    return 0;
  pa_rt_set_error("%s: %d rows, %d history columns (1 .. 16) against %d columns (1 .. 16), ring of %d slots from slot %d, "
                  "leading dimension %d", what, n, K, q, cap, head, ldh);
  return 1;
}

// the two blocks of a fold lie behind word 0, inside the buffer, and apart
inline int red_blocks_bad(const hist_block_t& a, const hist_block_t& b) {
  const int na = a.rows * a.cols, nb = b.rows * b.cols;
  if (a.rows < 0 || a.rows > HIST_MAX || a.cols < 0 || a.cols > HIST_MAX || b.rows < 0 || b.rows > HIST_MAX || b.cols < 0 ||
      b.cols > HIST_MAX)
    return 1;
  if (na > 0 && (a.off < 1 || a.off + na > HIST_RED_WORDS)) return 1;
  if (nb > 0 && (b.off < 1 || b.off + nb > HIST_RED_WORDS)) return 1;
  if (na > 0 && nb > 0 && a.off < b.off + nb && b.off < a.off + na) return 1;
  return 0;
}

}  // namespace

extern "C" {

size_t pa_k_hist_part_doubles(void) { return (size_t)HIST_MAX_BLOCKS * HIST_PART; }

int pa_k_hist_dots(int n, int K, int q, const double* Xh, int ldh, int head, int cap, const double* W, int ldw,
                   double* part, double* out) {
  if (hist_args_bad("pa_k_hist_dots", n, K, q, ldh, head, cap)) return 1;
  if (!Xh || !W || !part || !out || ldw < n) {
    pa_rt_set_error("pa_k_hist_dots: a NULL array, or leading dimension %d below the %d rows", ldw, n);
    return 1;
  }
  const int blocks = hist_blocks(n);
  PA_LAUNCH((k_hist_dots<false>), dim3(blocks, (q + HIST_QT - 1) / HIST_QT), dim3(WG), 0, cur_stream(), (size_t)n, K, q,
            Xh, (size_t)ldh, head, cap, (const int*)nullptr, (const double*)nullptr, W, (size_t)ldw, part);
  PA_LAUNCH(k_hist_fold, dim3(1), dim3(HIST_PART), 0, cur_stream(), blocks, K, q, part, out);
  return kfail("k_hist_dots");
}

int pa_k_hist_dots_mapped(int m, int K, int q, const double* Xh, int ldh, int head, int cap, const int* src,
                          const double* dl, const double* Wp, int ts, double* part, double* out) {
  if (hist_args_bad("pa_k_hist_dots_mapped", m, K, q, ldh, head, cap)) return 1;
  if (!Xh || !Wp || !src || !dl || !part || !out || ts < q) {
    pa_rt_set_error("pa_k_hist_dots_mapped: a NULL array, or a panel stride %d below the %d columns", ts, q);
    return 1;
  }
  const int blocks = hist_blocks(m);
  PA_LAUNCH((k_hist_dots<true>), dim3(blocks, (q + HIST_QT - 1) / HIST_QT), dim3(WG), 0, cur_stream(), (size_t)m, K, q,
            Xh, (size_t)ldh, head, cap, src, dl, Wp, (size_t)ts, part);
  PA_LAUNCH(k_hist_fold, dim3(1), dim3(HIST_PART), 0, cur_stream(), blocks, K, q, part, out);
  return kfail("k_hist_dots_mapped");
}

int pa_k_hist_combine(int n, int K, int q, const double* Xh, int ldh, int head, int cap, const double* c, double* X0,
                      int ldx0) {
  if (hist_args_bad("pa_k_hist_combine", n, K, q, ldh, head, cap)) return 1;
  if (!Xh || !c || !X0 || ldx0 < n) {
    pa_rt_set_error("pa_k_hist_combine: a NULL array, or leading dimension %d below the %d rows", ldx0, n);
    return 1;
  }
  PA_LAUNCH(k_hist_combine, dim3(combine_blocks(n)), dim3(WG), 0, cur_stream(), (size_t)n, K, q, Xh, (size_t)ldh, head,
            cap, c, X0, (size_t)ldx0);
  return kfail("k_hist_combine");
}

/* ---- owned rows (several processes) ---- */
size_t pa_k_hist_owned_part_doubles(void) { return 2 * (size_t)HIST_REGION; }

int pa_k_hist_gather(int m, int N, int q, const int* src, const double* a, int lda, const int* slots, int cap, double* out,
                     int ldo) {
  hist_slots_t sl;
  int ok = m >= 0 && N >= m && q >= 1 && q <= HIST_MAX && cap >= 1 && cap <= HIST_MAX && lda >= N && ldo >= m && src && a && out;
  for (int j = 0; j < HIST_MAX; ++j) {
    sl.s[j] = j < q ? (slots ? slots[j] : j) : -1;
    if (sl.s[j] >= cap) ok = 0;
  }
  if (!ok) {
    pa_rt_set_error("pa_k_hist_gather: %d of %d rows, %d columns (1 .. 16) into %d slots (each below the slot count), "
                    "leading dimensions %d / %d, or a NULL array", m, N, q, cap, lda, ldo);
    return 1;
  }
  PA_LAUNCH(k_hist_gather, dim3(combine_blocks(m)), dim3(WG), 0, cur_stream(), (size_t)m, q, src, a, (size_t)lda, sl, out,
            (size_t)ldo);
  return kfail("k_hist_gather");
}

int pa_k_hist_ring_scaled(int m, int K, const double* Xl, int ldh, const double* dl, double* out, int ldo) {
  if (m < 0 || K < 1 || K > HIST_MAX || ldh < m || ldo < m || !Xl || !dl || !out) {
    pa_rt_set_error("pa_k_hist_ring_scaled: %d rows, %d columns (1 .. 16), leading dimensions %d / %d, or a NULL array", m, K,
                    ldh, ldo);
    return 1;
  }
  PA_LAUNCH(k_hist_ring_scaled, dim3(combine_blocks(m)), dim3(WG), 0, cur_stream(), (size_t)m, K, Xl, (size_t)ldh, dl, out,
            (size_t)ldo);
  return kfail("k_hist_ring_scaled");
}

/* K = 0, an empty ring, is taken: the sums b_j^2 are still formed */
int pa_k_hist_project_owned(int m, int N, int K, int q, const double* Xl, int ldh, int head, int cap, const int* src,
                            const double* b, int ldb, double* part, double* red, int off_bb, int off_g) {
  if (K != 0 && hist_args_bad("pa_k_hist_project_owned", m, K, q, ldh, head, cap)) return 1;
  const hist_block_t bb = {1, 1, q, off_bb}, g = {0, K, q, off_g};
  if (m < 0 || N < m || K < 0 || q < 1 || q > HIST_MAX || (K > 0 && !Xl) || !src || !b || !part || !red || ldb < N ||
      red_blocks_bad(bb, g)) {
    pa_rt_set_error("pa_k_hist_project_owned: %d of %d rows, %d history columns (0 .. 16) against %d columns (1 .. 16), a "
                    "NULL array, leading dimension %d below the rows, or blocks at %d / %d outside the %d words", m, N, K, q,
                    ldb, off_bb, off_g, HIST_RED_WORDS);
    return 1;
  }
  const int blocks = hist_blocks(m);
  PA_LAUNCH((k_hist_dots_owned<false>), dim3(blocks, (q + HIST_QT - 1) / HIST_QT, 1), dim3(WG), 0, cur_stream(), (size_t)m,
            K, q, Xl, (size_t)ldh, head, K > 0 ? cap : 1, (const double*)nullptr, (size_t)0, src, (const double*)nullptr, b,
            (size_t)ldb, part);
  PA_LAUNCH(k_hist_fold_red, dim3(1), dim3(2 * HIST_PART), 0, cur_stream(), blocks, part, bb, g, red);
  return kfail("k_hist_project_owned");
}

/* Xn == NULL: the block DO alone (the refresh: q = K columns of the panel against the ring); K = 0 with Xn: DN alone */
int pa_k_hist_gram_owned(int m, int K, int q, const double* Xl, int ldh, int head, int cap, const double* Xn, int ldn,
                         const double* dl, const double* Wp, int ts, double* part, double* red, int off_do, int off_dn) {
  if (K != 0 && hist_args_bad("pa_k_hist_gram_owned", m, K, q, ldh, head, cap)) return 1;
  const hist_block_t d_o = {0, K, q, off_do}, d_n = {1, Xn ? q : 0, Xn ? q : 0, off_dn};
  if (m < 0 || K < 0 || (K == 0 && !Xn) || q < 1 || q > HIST_MAX || (K > 0 && !Xl) || (Xn && ldn < m) || !dl || !Wp || !part ||
      !red || ts < q || red_blocks_bad(d_o, d_n)) {
    pa_rt_set_error("pa_k_hist_gram_owned: %d rows, %d history columns (0 .. 16) against %d columns (1 .. 16), a NULL array, "
                    "a panel stride %d below the columns, leading dimension %d below the rows, or blocks at %d / %d "
                    "outside the %d words", m, K, q, ts, ldn, off_do, off_dn, HIST_RED_WORDS);
    return 1;
  }
  const int blocks = hist_blocks(m);
  PA_LAUNCH((k_hist_dots_owned<true>), dim3(blocks, (q + HIST_QT - 1) / HIST_QT, Xn ? 2 : 1), dim3(WG), 0, cur_stream(),
            (size_t)m, K, q, Xl, (size_t)ldh, head, K > 0 ? cap : 1, Xn, (size_t)ldn, (const int*)nullptr, dl, Wp, (size_t)ts,
            part);
  PA_LAUNCH(k_hist_fold_red, dim3(1), dim3(2 * HIST_PART), 0, cur_stream(), blocks, part, d_o, d_n, red);
  return kfail("k_hist_gram_owned");
}

int pa_k_hist_combine_owned(int m, int N, int K, int q, const double* Xl, int ldh, int head, int cap, const double* c,
                            const int* src, double* X0, int ldx0) {
  /* K = 0, an empty ring: zeros at the owned rows */
  if (K != 0 && hist_args_bad("pa_k_hist_combine_owned", m, K, q, ldh, head, cap)) return 1;
  if (m < 0 || K < 0 || q < 1 || q > HIST_MAX || (K > 0 && (!Xl || !c)) || !src || !X0 || N < m || ldx0 < N) {
    pa_rt_set_error("pa_k_hist_combine_owned: %d of %d rows, %d history columns (0 .. 16) into %d columns (1 .. 16), a NULL "
                    "array, or leading dimension %d below the rows", m, N, K, q, ldx0);
    return 1;
  }
  PA_LAUNCH(k_hist_combine_owned, dim3(combine_blocks(m)), dim3(WG), 0, cur_stream(), (size_t)m, K, q, Xl, (size_t)ldh, head,
            K > 0 ? cap : 1, c, src, X0, (size_t)ldx0);
  return kfail("k_hist_combine_owned");
}

}  // extern "C"
