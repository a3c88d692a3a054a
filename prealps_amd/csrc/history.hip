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

}  // extern "C"
