// dense_device.h -- what more than one of the dense panel units (dense_gram.hip, dense_update.hip,
// dense_panels.hip, dense_system.hip) uses: the workgroup-wide Cholesky / alpha step, the column sums of a workgroup, the note to
// a polling host, the fixed tree of the per-system sums, and the launch grids.
// Private to those units; like kernels_common.h every unit gets its own copy.
#pragma once
#include "kernels_common.h"

namespace {

// The lanes of ONE wavefront see each other's LDS stores once both of these have been passed (DS operations of
// a wavefront execute in order; this keeps the compiler from moving them and drains the counter).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// In-place upper Cholesky of the t x t column-major W in LDS (LAPACK dpotf2 'U': on failure
// the failing pivot is stored and the rest of W is left untouched), called by a whole
// workgroup; t <= 16.  The first wavefront does the work, right looking: pivot j, row j of U in
// parallel over the lanes, then the rank-1 update of the trailing triangle, t^2 / 64 entries per lane --
// three LDS round trips per pivot instead of the t^3 / 3 dependent LDS reads of one thread walking
// dpotf2's loops (21 us per iteration at 8 columns, round 3).  Every entry sees the same operations in
// the same order as in dpotf2 (the terms u_kj u_ki are taken off one k after the other, then one
// division), so the factor is bitwise the same; a pivot that is not positive -- rare, and by then the
// trailing entries are no longer dpotf2's -- sends one thread through dpotf2's own loops on a copy.
__device__ __forceinline__ void potrf_upper_wg(double* W, int t, int* info) {
  __shared__ double keep[256];
  __shared__ int s_fail;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    for (int e = lane; e < t * t; e += 64) keep[e] = W[e];
    int fail = 0;
    // the lane's (up to four) entries of the upper triangle: row / column worked out once (a division by the
    // run-time t costs more than a pivot step)
    int er[4], ec[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = lane + 64 * q;
      ec[q] = e / t; er[q] = e - ec[q] * t;
      if (e >= t * t || er[q] > ec[q]) er[q] = -1;      // (below the diagonal or beyond the block: never touched)
    }
    wave_lds_sync();
    for (int j = 0; j < t; ++j) {
      double d = W[j + t * j];
      if (!(d > 0.0)) { fail = j + 1; break; }       // (the same value in every lane)
      d = sqrt(d);
      double u = 0.0;
      if (lane > j && lane < t) u = W[j + t * lane] / d;
      wave_lds_sync();
      if (lane == j) W[j + t * j] = d;
      if (lane > j && lane < t) W[j + t * lane] = u;
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (er[q] > j) W[lane + 64 * q] -= W[j + t * er[q]] * W[j + t * ec[q]];
      wave_lds_sync();
    }
    if (fail) {
      for (int e = lane; e < t * t; e += 64) W[e] = keep[e];
      wave_lds_sync();
      if (lane == 0) {
        fail = 0;
        for (int j = 0; j < t; ++j) {
          double d = W[j + t * j];
          for (int k = 0; k < j; ++k) d -= W[k + t * j] * W[k + t * j];
          if (!(d > 0.0)) { W[j + t * j] = d; fail = j + 1; break; }
          d = sqrt(d);
          W[j + t * j] = d;
          for (int i = j + 1; i < t; ++i) {
            double sv = W[j + t * i];
            for (int k = 0; k < j; ++k) sv -= W[k + t * j] * W[k + t * i];
            W[j + t * i] = sv / d;
          }
        }
        s_fail = fail;
      }
    } else if (lane == 0) s_fail = 0;
    if (lane == 0 && info) *info = s_fail;
  }
  __syncthreads();
}

// [W ; G^T] ((t+T) x t, ld t+T) -> mu = chol(W) (t x t, ld t), alpha = U^-T G (t x T, ld t);
// called by a whole workgroup, W / G = 256 doubles of LDS each.  (ecg.c:431 + :438 with the
// Gram of the un-normalised P: (P U^-1)^T R = U^-T (P^T R).)
__device__ __forceinline__ void potrf_alpha_wg(const double* buf, int t, int T, double* mu,
                                               double* alpha, int* info, double* W, double* G) {
  const int ld = t + T, nt = blockDim.x;
  for (int e = threadIdx.x; e < t * t; e += nt) W[e] = buf[(e % t) + ld * (e / t)];
  for (int e = threadIdx.x; e < t * T; e += nt) { const int i = e % t, c = e / t; G[e] = buf[(t + c) + ld * i]; }
  __syncthreads();
  potrf_upper_wg(W, t, info);
  // forward substitution with U^T on the T columns of G at once, by the first wavefront: row i is divided by
  // its pivot, then taken off the rows below (t T / 64 entries per lane) -- per entry the operations and the
  // order of one lane walking its column (g_i - u_0i a_0 - u_1i a_1 ... , then the division)
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int gk[4], gc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = lane + 64 * q;
      gc[q] = e / t; gk[q] = e - gc[q] * t;
      if (e >= t * T) gk[q] = -1;
    }
    for (int i = 0; i < t; ++i) {
      const double d = W[i + t * i];
      if (lane < T) G[i + t * lane] = G[i + t * lane] / d;
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (gk[q] > i) G[lane + 64 * q] -= W[i + t * gk[q]] * G[i + t * gc[q]];
      wave_lds_sync();
    }
  }
  __syncthreads();
  // (mu / alpha / info may be null: the factor and alpha stay in W and G for the caller)
  if (mu) for (int e = threadIdx.x; e < t * t; e += nt) mu[e] = W[e];
  if (alpha) for (int e = threadIdx.x; e < t * T; e += nt) alpha[e] = G[e];
}

template <int TS>
__device__ __forceinline__ void block_sum_cols(double (&v)[TS], double* __restrict__ out) {
  __shared__ double red[WG / 64][TS];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1)
#pragma unroll
    for (int c = 0; c < TS; ++c) v[c] += __shfl_xor(v[c], off);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < TS; ++c) red[wave][c] = v[c];
  __syncthreads();
  if (threadIdx.x < TS) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < WG / 64; ++w) s += red[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// Two words the host is waiting for go out to pinned memory from a kernel that runs anyway (no copy, no extra
// launch); host[2] = seq (when given) tells a polling host that the two words are there (pa_k_note_seq).  One lane.
__device__ __forceinline__ void note_to_host(double* host, const double* src, double seq) {
  __hip_atomic_store(host, src[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(host + 1, src[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  if (seq != 0.0) __hip_atomic_store(host + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The per-system sums of the stopping test: the sum over the s columns of system j (ascending) of the sum over the
// blocks of rtr[blk*ts + c] (the column sums of R^2 an update kernel or k_colnorm2 left).  One workgroup; 16 threads
// per column take the blocks b = l, l + 16, ... in turn and are folded by a fixed tree, so the k values are
// reproducible.  group_fold: that sum in thread j < k (0 elsewhere); called by the whole workgroup, red: WG doubles.
__device__ __forceinline__ double group_fold(const double* __restrict__ rtr, int nblk, int ts, int k, int s, double* red) {
  const int c = threadIdx.x >> 4, l = threadIdx.x & 15;
  double v = 0.0;
  if (c < k * s)
    for (int b = l; b < nblk; b += 16) v += rtr[(size_t)b * ts + c];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = 8; off > 0; off >>= 1) {
    if (l < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  double g = 0.0;
  if (threadIdx.x < k)
    for (int q = 0; q < s; ++q) g += red[(threadIdx.x * s + q) << 4];
  return g;
}

inline int grid_rows(int m, int per_thread_rows = 1) {
  long long blocks = ((long long)m + (long long)WG * per_thread_rows - 1) / ((long long)WG * per_thread_rows);
  if (blocks < 1) blocks = 1;
  const long long cap = 2048;
  return (int)(blocks < cap ? blocks : cap);
}

/* The grid of a kernel that leaves one partial block or one row of column sums per workgroup (k_trsm_update and
 * k_update_xrz: two rows per lane): the layout of those sums (and so the norm summed from them) depends on it. */
inline int update_grid(int m, int rows_per_lane = 2, int cap = GRAM_MAX_BLOCKS) {
  const int blocks = grid_rows(m, rows_per_lane);
  return blocks > cap ? cap : blocks;
}

}  // namespace
