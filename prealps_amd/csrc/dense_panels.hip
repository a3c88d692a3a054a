// dense_panels.hip -- the column utilities of the ECG block iteration (copy, right multiplication, permutation, row
// sums), the starts and finishes of several systems and of an initial guess, the HBM probes and the spacer of the
// phase timers, with their C launchers (pa_device.h).  See dense_gram.hip for the layout of panels.
#include "dense_device.h"

namespace {
// ------------------------------------------------ HBM calibration ----
// What this device sustains on the plainest streaming kernels, measured in the same process
// as the solver kernels (bench.py quotes the SpMM against the 8 TB/s spec and against this).
__global__ __launch_bounds__(WG) void k_probe_copy(size_t n2, const double2* __restrict__ src,
                                                   double2* __restrict__ dst) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n2; i += stride) dst[i] = src[i];
}
__global__ __launch_bounds__(WG) void k_probe_read(size_t n2, const double2* __restrict__ src,
                                                   double* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * WG;
  double s = 0.0;
#pragma unroll 4
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n2; i += stride) { const double2 v = src[i]; s += v.x + v.y; }
  if (s == 12345.678) out[0] = s;   // keeps the loads alive, never true for the zero-filled buffer
}

template <int TS>
__global__ __launch_bounds__(WG) void k_copy_cols(int m, int nc, const double* __restrict__ src,
                                                  double* __restrict__ dst) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double s[TS], d[TS];
    load_row<TS>(src, row, s);
    load_row<TS>(dst, row, d);
#pragma unroll
    for (int c = 0; c < TS; ++c) if (c < nc) d[c] = s[c];
    store_row<TS>(dst, row, d);
  }
}

template <int TS>
__global__ __launch_bounds__(WG) void k_right_mult(int m, int t, const double* __restrict__ Q,
                                                   double* __restrict__ A) {
  __shared__ double sq[TS * TS];
  for (int e = threadIdx.x; e < t * t; e += WG) sq[e] = Q[e];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double a[TS], o[TS];
    load_row<TS>(A, row, a);
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      o[c] = a[c];
      if (c < t) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < TS; ++k) if (k < t) s = fma(a[k], sq[k + t * c], s);
        o[c] = s;
      }
    }
    store_row<TS>(A, row, o);
  }
}

template <int TS>
__global__ __launch_bounds__(WG) void k_permute_cols(int m, int n, const int* __restrict__ piv,
                                                     double* __restrict__ A) {
  __shared__ int sp[TS];
  if (threadIdx.x < n) sp[threadIdx.x] = piv[threadIdx.x];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double a[TS], o[TS];
    load_row<TS>(A, row, a);
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      o[c] = a[c];
      if (c < n) {
        const int s = sp[c];
        double v = a[0];
#pragma unroll
        for (int k = 1; k < TS; ++k) v = (s == k) ? a[k] : v;
        o[c] = v;
      }
    }
    store_row<TS>(A, row, o);
  }
}

// BF-Omin (ecg.c:358-393 of the reference: copy Z -> P, dlapmt, dtrsm on the leading `t` columns) in one pass:
// dst(:, c) = src(:, piv[c]) for c < n, then the first t columns times U^-1 -- the substitution of k_trsm, same
// order of operations, so the result equals the three kernels' bit for bit.
template <int TS>
__global__ __launch_bounds__(WG) void k_permute_trsm(int m, int n, const int* __restrict__ piv, int t,
                                                     const double* __restrict__ U, const double* __restrict__ src,
                                                     double* __restrict__ dst) {
  __shared__ double su[TS * TS];
  __shared__ double sd[TS];
  __shared__ int sp[TS];
  for (int e = threadIdx.x; e < t * t; e += WG) su[e] = U[e];
  if (threadIdx.x < n) sp[threadIdx.x] = piv[threadIdx.x];
  __syncthreads();
  if (threadIdx.x < t) sd[threadIdx.x] = 1.0 / su[threadIdx.x + t * threadIdx.x];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double a[TS], p[TS];
    load_row<TS>(src, row, a);
    if (n < TS) load_row<TS>(dst, row, p);      // (columns beyond the panel's width stay what they are)
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      if (c < n) {
        const int s_ = sp[c];
        double v = a[0];
#pragma unroll
        for (int k = 1; k < TS; ++k) v = (s_ == k) ? a[k] : v;
        p[c] = v;
      }
    }
#pragma unroll
    for (int j = 0; j < TS; ++j) {
      if (j < t) {
        double s_ = p[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s_ = fma(-p[k], su[k + t * j], s_);
        p[j] = s_ * sd[j];
      }
    }
    store_row<TS>(dst, row, p);
  }
}

template <int TS>
__global__ __launch_bounds__(WG) void k_rowsum(int m, int nc, const double* __restrict__ X,
                                               double* __restrict__ sol) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double x[TS];
    load_row<TS>(X, row, x);
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < TS; ++c) if (c < nc) s += x[c];
    sol[row] = s;
  }
}

// ---- several right-hand sides (preAlps_ECGInitializeMulti / FinalizeMulti) ----
// The start: system j owns the columns j*s .. j*s + s - 1 of the panel, and a row of part p puts B(row, j) into
// column j*s + (p % s) (pcol[row] = p % s); every other entry of R0 is zero.  Each workgroup leaves the sums of
// B(:, j)^2 over its rows in sums[blk*TS + j], the layout of k_colnorm2, for k_group_norms.
template <int TS>
__global__ __launch_bounds__(WG) void k_multi_start(int m, int k, int s, const double* __restrict__ B, size_t ldb,
                                                    const int* __restrict__ pcol, double* __restrict__ R,
                                                    double* __restrict__ sums) {
  double acc[TS];
#pragma unroll
  for (int j = 0; j < TS; ++j) acc[j] = 0.0;
  const int nc = k * s;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    const int pc = pcol[row];
    double r[TS];
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      const int j = c / s;
      r[c] = (c < nc && c - j * s == pc) ? B[row + (size_t)j * ldb] : 0.0;
    }
    store_row<TS>(R, row, r);
#pragma unroll
    for (int j = 0; j < TS; ++j)
      if (j < k) { const double v = B[row + (size_t)j * ldb]; acc[j] = fma(v, v, acc[j]); }
  }
  block_sum_cols<TS>(acc, sums + (size_t)blockIdx.x * TS);
}

// ---- a start from an initial guess (preAlps_ECGInitializeGuess) ----
// X0 as a panel, by the placement rule of k_multi_start: X(row, j*s + pcol[row]) = X0(row, j), zero elsewhere, so the
// sum of the columns of system j is X0(row, j) itself.
template <int TS>
__global__ __launch_bounds__(WG) void k_guess_split(int m, int k, int s, const double* __restrict__ X0, size_t ld,
                                                    const int* __restrict__ pcol, double* __restrict__ X) {
  const int nc = k * s;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    const int pc = pcol[row];
    double x[TS];
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      const int j = c / s;
      x[c] = (c < nc && c - j * s == pc) ? X0[row + (size_t)j * ld] : 0.0;
    }
    store_row<TS>(X, row, x);
  }
}

// R0 from the product AX = A X0 of that panel: r0_j = B(row, j) - (the sum of the columns of system j of AX, added in
// ascending order), split by the same rule.  Each workgroup leaves the sums of B(:, j)^2 over its rows in
// bsums[blk*TS + j] (the accumulation and the layout of k_multi_start, so the same bits) and the sums of R0(:, c)^2 in
// rsums[blk*TS + c] (the layout of k_colnorm2), both for k_group_norms.
template <int TS>
__global__ __launch_bounds__(WG) void k_guess_start(int m, int k, int s, const double* __restrict__ B, size_t ldb,
                                                    const int* __restrict__ pcol, const double* __restrict__ AX,
                                                    double* __restrict__ R, double* __restrict__ bsums,
                                                    double* __restrict__ rsums) {
  double accb[TS], accr[TS];
#pragma unroll
  for (int j = 0; j < TS; ++j) { accb[j] = 0.0; accr[j] = 0.0; }
  const int nc = k * s;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    const int pc = pcol[row];
    double g[TS], r[TS];
    load_row<TS>(AX, row, g);
    // g[c] <- the sum of its system's columns: a running sum up to the last column of each system ...
    double run = 0.0;
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < TS; ++c)
      if (c < nc) {
        run += g[c];
        g[c] = run;
        if (++cnt == s) { run = 0.0; cnt = 0; }
      }
    // ... handed down to the columns before it
    double sum = 0.0;
    cnt = 0;
#pragma unroll
    for (int c = TS - 1; c >= 0; --c)
      if (c < nc) {
        if (cnt == 0) sum = g[c];
        if (++cnt == s) cnt = 0;
        const int j = c / s;
        r[c] = (c - j * s == pc) ? B[row + (size_t)j * ldb] - sum : 0.0;
        accr[c] = fma(r[c], r[c], accr[c]);
      } else r[c] = 0.0;
    store_row<TS>(R, row, r);
#pragma unroll
    for (int j = 0; j < TS; ++j)
      if (j < k) { const double v = B[row + (size_t)j * ldb]; accb[j] = fma(v, v, accb[j]); }
  }
  block_sum_cols<TS>(accb, bsums + (size_t)blockIdx.x * TS);
  __syncthreads();      // (block_sum_cols keeps one LDS buffer: its readers are done before the second pass writes)
  block_sum_cols<TS>(accr, rsums + (size_t)blockIdx.x * TS);
}

// (group_fold, the fixed tree of the per-system sums: dense_device.h)
// One process: the values go to device memory and to pinned host words, which the host reads once the launch or
// event behind this one has completed (it keys on nothing this kernel writes).
__global__ __launch_bounds__(WG) void k_group_norms(const double* __restrict__ rtr, int nblk, int ts, int k, int s,
                                                    double* __restrict__ out, double* host) {
  __shared__ double red[WG];
  const double g = group_fold(rtr, nblk, ts, k, s, red);
  if (threadIdx.x < k) {
    out[threadIdx.x] = g;
    if (host) __hip_atomic_store(host + threadIdx.x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence_system();
}

// Several processes: the k sums are this process's share, so they go neither to the host nor to a buffer of their
// own but behind the two words a collective of the iteration carries anyway: buf[0] = the local sum of squares of all
// of R (g_0 + g_1 + ... in ascending j), buf[1] = the Cholesky status (*info, what k_trace_finish puts there),
// buf[2 + j] = g_j.  One all-reduce of 2 + k words (or of the block in front of buf and these) then leaves the global
// values on every process.
__global__ __launch_bounds__(WG) void k_group_norms_ride(const double* __restrict__ rtr, int nblk, int ts, int k, int s,
                                                         const int* __restrict__ info, double* __restrict__ buf) {
  __shared__ double red[WG];
  __shared__ double grp[16];
  const double g = group_fold(rtr, nblk, ts, k, s, red);
  if (threadIdx.x < k) {
    grp[threadIdx.x] = g;
    buf[2 + threadIdx.x] = g;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double all = 0.0;
    for (int j = 0; j < k; ++j) all += grp[j];
    buf[0] = all;
    buf[1] = info ? (double)info[0] : 0.0;
  }
}

// The finish: sol[row + j*ld] = sum of X(row, c) over the columns of system j, added in ascending c as k_rowsum does.
template <int TS>
__global__ __launch_bounds__(WG) void k_rowsum_groups(int m, int k, int s, const double* __restrict__ X,
                                                      double* __restrict__ sol, size_t ld) {
  const int nc = k * s;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double x[TS];
    load_row<TS>(X, row, x);
    double acc = 0.0;
    int j = 0, cnt = 0;
#pragma unroll
    for (int c = 0; c < TS; ++c)
      if (c < nc) {
        acc += x[c];
        if (++cnt == s) { sol[row + (size_t)j * ld] = acc; acc = 0.0; cnt = 0; ++j; }
      }
  }
}

}  // namespace

extern "C" {

/* One wavefront that does nothing for `us` microseconds (phase timers, context.c: the launch of a timed region is
 * already queued when the spacer ends, so the event pair around it measures the kernels and not the dispatch
 * latency of a launch onto an idle stream). */
__global__ void k_spacer(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
int pa_k_spacer(int us) {
  PA_LAUNCH(k_spacer, dim3(1), dim3(64), 0, cur_stream(), (long long)us * 100);     /* (100 MHz counter) */
  return kfail("k_spacer");
}

int pa_k_probe(int which, size_t bytes, const double* src, double* dst) {
  const size_t n2 = bytes / 16;
  if (which == 0) PA_LAUNCH(k_probe_copy, dim3(8192), dim3(WG), 0, cur_stream(), n2, (const double2*)src, (double2*)dst);
  else PA_LAUNCH(k_probe_read, dim3(8192), dim3(WG), 0, cur_stream(), n2, (const double2*)src, dst);
  return kfail("k_probe");
}

int pa_k_copy_cols(int m, int ts, int nc, const double* src, double* dst) {
  if (nc <= 0) return 0;
  TS_DISPATCH(ts, PA_LAUNCH((k_copy_cols<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0,
                                     cur_stream(), m, nc, src, dst));
  return kfail("k_copy_cols");
}

int pa_k_right_mult(int m, int ts, int t, const double* Q, double* A) {
  if (t <= 0) return 0;
  TS_DISPATCH(ts, PA_LAUNCH((k_right_mult<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0,
                                     cur_stream(), m, t, Q, A));
  return kfail("k_right_mult");
}

int pa_k_permute_trsm(int m, int ts, int n, const int* piv, int t, const double* U, const double* src, double* dst) {
  if (m <= 0) return 0;
  TS_DISPATCH(ts, PA_LAUNCH((k_permute_trsm<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0, cur_stream(), m, n, piv, t, U,
                            src, dst));
  return kfail("k_permute_trsm");
}

int pa_k_permute_cols(int m, int ts, int n, const int* piv, double* A) {
  if (n <= 0) return 0;
  TS_DISPATCH(ts, PA_LAUNCH((k_permute_cols<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0,
                                     cur_stream(), m, n, piv, A));
  return kfail("k_permute_cols");
}

int pa_k_rowsum(int m, int ts, int nc, const double* X, double* sol) {
  TS_DISPATCH(ts, PA_LAUNCH((k_rowsum<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0,
                                     cur_stream(), m, nc, X, sol));
  return kfail("k_rowsum");
}

static int multi_args_bad(const char* what, int ts, int k, int s) {
  if (k >= 1 && s >= 1 && k * s <= ts && ts <= 16) return 0;
  pa_rt_set_error("%s: %d systems of %d columns do not fit a panel of stride %d", what, k, s, ts);
  return 1;
}

int pa_k_multi_start(int m, int ts, int k, int s, const double* B, int ldb, const int* pcol, double* R,
                     double* sums, int* nblk) {
  if (multi_args_bad("pa_k_multi_start", ts, k, s)) return 1;
  const int blocks = update_grid(m, 4);
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_multi_start<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m, k, s, B, (size_t)ldb,
                            pcol, R, sums));
  return kfail("k_multi_start");
}

int pa_k_guess_split(int m, int ts, int k, int s, const double* X0, int ld, const int* pcol, double* X) {
  if (multi_args_bad("pa_k_guess_split", ts, k, s)) return 1;
  TS_DISPATCH(ts, PA_LAUNCH((k_guess_split<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0, cur_stream(), m, k, s, X0,
                            (size_t)ld, pcol, X));
  return kfail("k_guess_split");
}

int pa_k_guess_start(int m, int ts, int k, int s, const double* B, int ldb, const int* pcol, const double* AX,
                     double* R, double* bsums, double* rsums, int* nblk) {
  if (multi_args_bad("pa_k_guess_start", ts, k, s)) return 1;
  const int blocks = update_grid(m, 4);      // (the grid of pa_k_multi_start: the same partial sums of B^2)
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_guess_start<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m, k, s, B, (size_t)ldb,
                            pcol, AX, R, bsums, rsums));
  return kfail("k_guess_start");
}

int pa_k_group_norms(const double* rtr_partials, int nblk, int ts, int k, int s, double* out, double* host) {
  if (multi_args_bad("pa_k_group_norms", ts, k, s)) return 1;
  PA_LAUNCH(k_group_norms, dim3(1), dim3(WG), 0, cur_stream(), rtr_partials, nblk, ts, k, s, out, host);
  return kfail("k_group_norms");
}

int pa_k_group_norms_ride(const double* rtr_partials, int nblk, int ts, int k, int s, const int* info, double* buf) {
  if (multi_args_bad("pa_k_group_norms_ride", ts, k, s)) return 1;
  if (!buf) { pa_rt_set_error("pa_k_group_norms_ride: no buffer for the %d sums", k); return 1; }
  PA_LAUNCH(k_group_norms_ride, dim3(1), dim3(WG), 0, cur_stream(), rtr_partials, nblk, ts, k, s, info, buf);
  return kfail("k_group_norms_ride");
}

int pa_k_rowsum_groups(int m, int ts, int k, int s, const double* X, double* sol, int ld) {
  if (multi_args_bad("pa_k_rowsum_groups", ts, k, s)) return 1;
  TS_DISPATCH(ts, PA_LAUNCH((k_rowsum_groups<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0, cur_stream(), m, k, s, X,
                            sol, (size_t)ld));
  return kfail("k_rowsum_groups");
}

}  // extern "C"
