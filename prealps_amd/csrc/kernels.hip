// kernels.hip -- CDNA4 (gfx950) kernels of the ECG block iteration and their
// C launchers (pa_device.h).  All panels are row-interleaved [rows][TS] fp64,
// all small t x t blocks column-major like the reference's work area.
//
// Every kernel here is HBM-bandwidth bound (SpMM: 0.67 flop/B at t = 4; the
// tall-skinny kernels t/8..t/4 flop/B against a ridge of ~10 flop/B), so the
// design rules are coalesced 16-B accesses, LDS staging where rows are reused,
// 64-wide shuffle reductions, and XCD-aware block order for the SpMM gathers.
//
// This unit holds the dense panel kernels only: Gram products and their finishes, trsm / update,
// update_z, the column utilities, the HBM probes (k_probe_*) and the spacer, with their launchers
// and the one-shot states g_note_seq and g_zpack.  The SpMM is spmm.hip, the band block solve of
// the preconditioner bj_band.hip (one-copy records: bj_g4.hip), the sparse block solve nd_*.hip.
#include "kernels_common.h"

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

// 16-column panels: the same Gram product on the f64 matrix cores.  One v_mfma_f64_16x16x4
// takes four panel rows: lane l supplies A[row l>>4][col l&15] and B[row l>>4][col l&15] --
// a wave-wide load of either operand is 512 contiguous bytes -- and accumulates
// C[i][j] = sum_rows A[row][i] B[row][j] (C/D map: col = lane&15, row = (lane>>4) + 4*reg).
// The register-tiled kernel above re-reads every panel segment from L1 four to eight times at
// this width (139 us for 395 MB); this one reads each byte once.  Same partial-block layout.
template <int NPAN>
__global__ __launch_bounds__(WG) void k_gram_mfma16(int m, const double* __restrict__ A0,
                                                    const double* __restrict__ A1,
                                                    const double* __restrict__ B,
                                                    double* __restrict__ partials) {
  constexpr int TS = 16, LDP = NPAN * TS;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int col = lane & 15, rsub = lane >> 4;
  mfma_d4 acc[NPAN];
#pragma unroll
  for (int p = 0; p < NPAN; ++p) acc[p] = mfma_d4{0.0, 0.0, 0.0, 0.0};
  const size_t nquad = ((size_t)m + 3) >> 2;
  const size_t qstride = (size_t)gridDim.x * (WG / 64);
  constexpr int U = 4;                                 // quads in flight per wavefront
  for (size_t q0 = (size_t)blockIdx.x * (WG / 64) + wave; q0 < nquad; q0 += U * qstride) {
    double a[U][NPAN], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t row = (q0 + u * qstride) * 4 + rsub;
      const bool ok = row < (size_t)m;
      b[u] = ok ? B[row * TS + col] : 0.0;
      a[u][0] = ok ? A0[row * TS + col] : 0.0;
      if (NPAN > 1) a[u][NPAN - 1] = ok ? A1[row * TS + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int p = 0; p < NPAN; ++p) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][p], b[u], acc[p], 0, 0, 0);
  }
  __shared__ double red[WG / 64][LDP * TS];
#pragma unroll
  for (int p = 0; p < NPAN; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(p * TS + rsub + 4 * r) + LDP * col] = acc[p][r];
  __syncthreads();
  for (int e = tid; e < LDP * TS; e += WG) {
    double sum = red[0][e];
#pragma unroll
    for (int w2 = 1; w2 < WG / 64; ++w2) sum += red[w2][e];
    partials[(size_t)blockIdx.x * (LDP * TS) + e] = sum;
  }
}

// 8-column panels: [A0 | A1] fills the 16 rows of one tile, B its first 8 columns.
template <int NPAN>
__global__ __launch_bounds__(WG) void k_gram_mfma8(int m, const double* __restrict__ A0,
                                                   const double* __restrict__ A1,
                                                   const double* __restrict__ B,
                                                   double* __restrict__ partials) {
  constexpr int TS = 8, LDP = NPAN * TS;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int col = lane & 15, rsub = lane >> 4;
  const double* __restrict__ Ap = (col < TS) ? A0 : A1;      // panel this lane's A column lives in
  const bool a_on = col < LDP, b_on = col < TS;
  const int ac = col & (TS - 1);
  mfma_d4 acc = mfma_d4{0.0, 0.0, 0.0, 0.0};
  const size_t nquad = ((size_t)m + 3) >> 2;
  const size_t qstride = (size_t)gridDim.x * (WG / 64);
  constexpr int U = 4;
  for (size_t q0 = (size_t)blockIdx.x * (WG / 64) + wave; q0 < nquad; q0 += U * qstride) {
    double a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t row = (q0 + u * qstride) * 4 + rsub;
      const bool ok = row < (size_t)m;
      a[u] = (ok && a_on) ? Ap[row * TS + ac] : 0.0;
      b[u] = (ok && b_on) ? B[row * TS + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
  }
  __shared__ double red[WG / 64][LDP * TS];
  if (b_on)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (rsub + 4 * r < LDP) red[wave][(rsub + 4 * r) + LDP * col] = acc[r];
  __syncthreads();
  for (int e = tid; e < LDP * TS; e += WG) {
    double sum = red[0][e];
#pragma unroll
    for (int w2 = 1; w2 < WG / 64; ++w2) sum += red[w2][e];
    partials[(size_t)blockIdx.x * (LDP * TS) + e] = sum;
  }
}

// ------------------------------------------------ small finishing steps ----
// Measured and rejected: letting the last workgroup of the producing kernel (ticket counter)
// do these sums.  The device-scope release every workgroup needs before taking its ticket
// writes the whole dirty L2 back on gfx950 (one L2 per XCD): +130 us per iteration.
// Sum the per-workgroup partial blocks (fixed order) and scatter the active
// sub-block into the reference's t x t layout.  BS threads, red = BS doubles.
template <int BS>
__device__ __forceinline__ void finish_sum(const double* partials, int nblk, int npan, int ts,
                                           int a_lo, int a_hi, int nb, double* out, int ld_out,
                                           double* red, int ner_cap = BS, int g0 = 0, int gstride = 1) {
  const int ldp = npan * ts;
  const int na = a_lo + a_hi;
  const int ne = na * nb;
  int ner = 1;
  while (ner < ne && ner < ner_cap) ner <<= 1;        // elements summed side by side
  const int nsl = BS / ner;                           // slices of the partial blocks per element
  const int tid = threadIdx.x;
  const int e0 = tid % ner, s = tid / ner;
  // groups of `ner` elements, dealt out to the workgroups of the launch
  for (int base = g0 * ner; base < ne; base += gstride * ner) {
    const int e = base + e0;
    double sum = 0.0;
    int i = 0, j = 0;
    if (e < ne) {
      i = e % na; j = e / na;
      const int src = (i < a_lo ? i : ts + (i - a_lo)) + ldp * j;
      const double* q = partials + src;
      const size_t bstride = (size_t)ldp * ts;
      int b = s;
      for (; b + 7 * nsl < nblk; b += 8 * nsl) {       // eight loads in flight, added in order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = q[(size_t)(b + u * nsl) * bstride];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += v[u];
      }
      for (; b < nblk; b += nsl) sum += q[(size_t)b * bstride];
    }
    red[tid] = sum;
    __syncthreads();
    if (s == 0 && e < ne) {
      double tot = 0.0;
      for (int q2 = 0; q2 < nsl; ++q2) tot += red[q2 * ner + e0];
      out[i + ld_out * j] = tot;
    }
    __syncthreads();
  }
}

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

// Residual norm from the per-workgroup column sums: fixed-order tree over WG threads.
// res2[1] carries the Cholesky status so the host fetches both with one copy; `host`
// (pinned, device-visible) receives the same two values when given.
__device__ __forceinline__ void trace_finish_wg(const double* rtr, int nblk, int ts, int nc,
                                                double* res2, const int* info, double* host,
                                                double* red, double seq = 0.0) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += WG)
    for (int c = 0; c < nc; ++c) s += rtr[(size_t)b * ts + c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = WG / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double r2 = red[0], st = info ? (double)info[0] : 0.0;
    res2[0] = r2; res2[1] = st;
    // host[2] = seq (when given) tells a polling host that the two words are there (pa_k_note_seq)
    if (host) {
      __hip_atomic_store(host, r2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(host + 1, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __threadfence_system();
      if (seq != 0.0) __hip_atomic_store(host + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---------------------------------------------------------------- Gram ----
// C = [A0 | A1]^T B over the local rows.  Each lane owns a TI x TI tile of C
// for a strided set of rows; NPAN*(TS/TI)^2 lanes cover one row.  Lanes are
// then folded with wavefront shuffles (64 wide), waves through LDS, and each
// workgroup writes one partial block (summed by k_finish in a fixed order, so
// results are bitwise reproducible).
template <int TS, int NPAN>
__global__ __launch_bounds__(WG) void k_gram(int m, const double* __restrict__ A0,
                                             const double* __restrict__ A1,
                                             const double* __restrict__ B,
                                             double* __restrict__ partials) {
  constexpr int TI = TS < 4 ? TS : 4;
  constexpr int TD = TS / TI;
  constexpr int LPR = NPAN * TD * TD;
  constexpr int LDP = NPAN * TS;
  const int tid = threadIdx.x;
  const int li = tid % LPR;
  const int pan = li / (TD * TD), ti = (li / TD) % TD, tj = li % TD;
  const double* __restrict__ A = (pan == 0) ? A0 : A1;
  double acc[TI][TI];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TI; ++j) acc[i][j] = 0.0;
  const size_t rstride = (size_t)gridDim.x * WG / LPR;
  for (size_t row = ((size_t)blockIdx.x * WG + tid) / LPR; row < (size_t)m; row += rstride) {
    double a[TI], b[TI];
    const double2* ap = reinterpret_cast<const double2*>(A + row * TS + ti * TI);
    const double2* bp = reinterpret_cast<const double2*>(B + row * TS + tj * TI);
#pragma unroll
    for (int i = 0; i < TI / 2; ++i) {
      double2 va = ap[i], vb = bp[i];
      a[2 * i] = va.x; a[2 * i + 1] = va.y;
      b[2 * i] = vb.x; b[2 * i + 1] = vb.y;
    }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TI; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
  }
  // fold the 64/LPR row groups of the wave
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TI; ++j) acc[i][j] += __shfl_xor(acc[i][j], off);
  __shared__ double red[WG / 64][LDP * TS];
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  if (lane < LPR) {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TI; ++j)
        red[wave][(pan * TS + ti * TI + i) + LDP * (tj * TI + j)] = acc[i][j];
  }
  __syncthreads();
  for (int e = tid; e < LDP * TS; e += WG) {
    double s = red[0][e];
#pragma unroll
    for (int w = 1; w < WG / 64; ++w) s += red[w][e];
    partials[(size_t)blockIdx.x * (LDP * TS) + e] = s;
  }
}

__global__ __launch_bounds__(1024) void k_finish(const double* __restrict__ partials, int nblk,
                                               int npan, int ts, int a_lo, int a_hi, int nb,
                                               double* __restrict__ out, int ld_out) {
  __shared__ double red[1024];
  // several workgroups (large blocks, 16-column panels): 64 elements at a time each
  if (gridDim.x > 1) finish_sum<1024>(partials, nblk, npan, ts, a_lo, a_hi, nb, out, ld_out, red, 64, blockIdx.x, gridDim.x);
  else finish_sum<1024>(partials, nblk, npan, ts, a_lo, a_hi, nb, out, ld_out, red);
}

// k_finish and k_trace_finish in one launch: the Gram block that is about to be all-reduced and,
// right behind it (res2), the squared residual norm from the column sums the update kernel left
// (same order of additions as k_trace_finish), so that one collective carries both.
__global__ __launch_bounds__(1024) void k_finish_trace(const double* __restrict__ partials, int nblk,
                                                     int npan, int ts, int a_lo, int a_hi, int nb,
                                                     double* __restrict__ out, int ld_out,
                                                     const double* __restrict__ rtr, int rtr_nblk, int nc,
                                                     double* __restrict__ res2, const int* __restrict__ info) {
  __shared__ double red[1024];
  finish_sum<1024>(partials, nblk, npan, ts, a_lo, a_hi, nb, out, ld_out, red);
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < WG) {
    double s = 0.0;
    for (int b = tid; b < rtr_nblk; b += WG)
      for (int c = 0; c < nc; ++c) s += rtr[(size_t)b * ts + c];
    red[tid] = s;
  }
  __syncthreads();
  for (int off = WG / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) { res2[0] = red[0]; res2[1] = info ? (double)info[0] : 0.0; }
}

// k_finish followed by k_potrf_alpha on its output, one launch (single-process runs, where no
// all-reduce sits between the two).
__global__ __launch_bounds__(1024) void k_finish_potrf_alpha(const double* __restrict__ partials,
                                                           int nblk, int npan, int ts, int t, int T,
                                                           double* out, double* __restrict__ mu,
                                                           double* __restrict__ alpha,
                                                           int* __restrict__ info) {
  __shared__ double red[1024];
  finish_sum<1024>(partials, nblk, npan, ts, t, T, t, out, t + T, red);
  __threadfence_block();
  __syncthreads();
  potrf_alpha_wg(out, t, T, mu, alpha, info, red, red + 256);
}

// Wide Gram blocks (panels of 8 / 16 columns: 128 / 512 doubles per partial block, 512 of them = 0.5 / 2 MB,
// which ONE workgroup needs 9 / 36 us to read -- k_finish_potrf_alpha took 17-21 us per iteration at 8 columns,
// k_finish x 2 + k_potrf_alpha + k_trace_finish 43 us at 16): FINW_WG workgroups sum a contiguous share of the
// blocks each, element by element, coalesced; the share goes out with device-scope stores, a ticket elects the
// last workgroup (k_finish32's protocol: no fence), which adds the shares in their fixed order, scatters the
// active sub-block into `out` as finish_sum does and, as asked, factors it (t > 0: k_finish_potrf_alpha) and /
// or sums the residual norm next to it (rtr: k_finish_trace).  The ticket lives behind the shares in `scratch`
// (per buffer, zero when the buffer is made, set back to zero by the last workgroup).
constexpr int FINW_WG = 32;
constexpr int GRAM_SCRATCH_BLOCKS = FINW_WG + 1;
__global__ __launch_bounds__(WG) void k_finish_wide(const double* __restrict__ partials, int nblk, int npan, int ts,
                                                    int a_lo, int a_hi, int nb, double* out, int ld_out,
                                                    double* scratch, int t, int T, double* __restrict__ mu,
                                                    double* __restrict__ alpha, int* __restrict__ info,
                                                    const double* __restrict__ rtr, int rtr_nblk, int rtr_nc,
                                                    double* __restrict__ res2) {
  __shared__ double red[512];
  __shared__ int s_last;
  const int NB = npan * ts * ts;                 // doubles per partial block (128, 256 or 512)
  const int tid = threadIdx.x;
  const int lpb = NB < WG ? NB : WG;             // lanes that cover one block side by side
  const int nsl = WG / lpb, ept = NB / lpb;      // blocks side by side; elements per lane (1 or 2)
  const int l = tid % lpb, sl = tid / lpb;
  const int per = (nblk + FINW_WG - 1) / FINW_WG;
  const int b0 = blockIdx.x * per, b1 = min(nblk, b0 + per);
  double acc[2] = {0.0, 0.0};
  {
    // eight blocks' loads in flight at a time (one after the other, each paid a trip to memory: 16 of them were
    // most of this kernel's 21 us at 16 columns); the additions keep their order
    const int second = ept > 1 ? lpb : 0;
    int b = b0 + sl;
    for (; b + 7 * nsl < b1; b += 8 * nsl) {
      double v[8][2];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double* __restrict__ q = partials + (size_t)(b + u * nsl) * NB + l;
        v[u][0] = q[0];
        v[u][1] = q[second];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { acc[0] += v[u][0]; acc[1] += v[u][1]; }
    }
    for (; b < b1; b += nsl) {
      const double* __restrict__ q = partials + (size_t)b * NB + l;
      acc[0] += q[0];
      acc[1] += q[second];
    }
  }
  // (behind the LARGEST shares this buffer can see, 2 ts^2 doubles each: a call with one panel must not look for
  // its ticket where a call with two panels leaves share data)
  unsigned* ticket = reinterpret_cast<unsigned*>(scratch + (size_t)FINW_WG * 2 * ts * ts);
  // the side-by-side slices of this workgroup (up to four), then the share
  if (nsl > 1) {
    if (sl > 0) red[(sl - 1) * lpb + l] = acc[0];
    __syncthreads();
    if (sl == 0) for (int k = 1; k < nsl; ++k) acc[0] += red[(k - 1) * lpb + l];
  }
  if (sl == 0) {
    __hip_atomic_store(scratch + (size_t)blockIdx.x * NB + l, acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ept > 1) __hip_atomic_store(scratch + (size_t)blockIdx.x * NB + lpb + l, acc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) s_last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1);
  __syncthreads();
  if (!s_last) return;
  {
    // every share, in order: the two halves of the workgroup take 32 shares each when a block is 128 doubles
    double tot[2] = {0.0, 0.0};
    const int g0 = sl * (FINW_WG / nsl), g1 = g0 + FINW_WG / nsl;
    // (sixteen / eight shares at a time, all loads of a round in flight: a device-scope load is a trip to memory)
    int g = g0;
    for (; g + 16 <= g1; g += 16) {
      double v[16][2];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        v[u][0] = __hip_atomic_load(scratch + (size_t)(g + u) * NB + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[u][1] = ept > 1 ? __hip_atomic_load(scratch + (size_t)(g + u) * NB + lpb + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) { tot[0] += v[u][0]; tot[1] += v[u][1]; }
    }
    for (; g < g1; g += 8) {
      double v[8][2];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u][0] = __hip_atomic_load(scratch + (size_t)(g + u) * NB + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[u][1] = ept > 1 ? __hip_atomic_load(scratch + (size_t)(g + u) * NB + lpb + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { tot[0] += v[u][0]; tot[1] += v[u][1]; }
    }
    __syncthreads();
    if (nsl > 1 && sl > 0) red[(sl - 1) * lpb + l] = tot[0];
    __syncthreads();
    if (sl == 0) {
      for (int k = 1; k < nsl; ++k) tot[0] += red[(k - 1) * lpb + l];
      // element e of the partial block = (row, column) of [panel 0 | panel 1]^T B: scatter the active part
      const int ldp = npan * ts, na = a_lo + a_hi;
#pragma unroll
      for (int qx = 0; qx < 2; ++qx) {
        if (qx < ept) {
          const int e = l + qx * lpb, r = e % ldp, j = e / ldp;
          const int i = r < ts ? (r < a_lo ? r : -1) : (r - ts < a_hi ? a_lo + (r - ts) : -1);
          if (i >= 0 && j < nb && i < na) out[i + (size_t)ld_out * j] = tot[qx];
        }
      }
    }
  }
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t > 0) {
    __threadfence_block();
    __syncthreads();
    potrf_alpha_wg(out, t, T, mu, alpha, info, red, red + 256);
  }
  if (rtr) {
    __syncthreads();
    trace_finish_wg(rtr, rtr_nblk, ts, rtr_nc, res2, info, nullptr, red);
  }
}

// The [W ; G^T] block of 4-column panels (8 x 4) from many partial blocks (one per workgroup of
// the SpMM that formed them; 1 MB on the headline problem, which one workgroup needs 24 us to
// read): FIN32_WG workgroups sum a contiguous share each (32-byte loads, 32 blocks side by
// side, fixed order) into scratch; the last one to finish (ticket counter) adds
// the shares in order and, t > 0, factors and forms alpha as k_finish_potrf_alpha does.
// The body, for workgroup `bid` of the FIN32_WG that share one sum (k_finish32: the grid; k_finish32_pair: half of it).
constexpr int FIN32_WG = 64;
__device__ __forceinline__ void finish32_wg(const double* __restrict__ partials, int nblk, double* scratch, int t,
                                            int T, double* out, double* __restrict__ mu, double* __restrict__ alpha,
                                            int* __restrict__ info, const double* __restrict__ rtr, int rtr_nblk,
                                            int rtr_ts, int rtr_nc, double* __restrict__ res2, int bid,
                                            double* red, int& s_last) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, e4 = tid & 7, sl = tid >> 3;
  const int per = (nblk + FIN32_WG - 1) / FIN32_WG;
  const int b0 = bid * per, b1 = min(nblk, b0 + per);
  const d4* __restrict__ q = reinterpret_cast<const d4*>(partials) + e4;
  d4 sum = {0.0, 0.0, 0.0, 0.0};
  // four blocks per thread in flight, the last round too (blocks beyond the share: the thread's first block
  // again, added as zero) -- with 4174 / 5670 partial blocks a share is 66 / 89 blocks, i.e. two or three per
  // thread: the remainder loop this replaces took them one memory round trip after the other
  for (int b = b0 + sl; b < b1; b += 4 * 32) {
    d4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = q[(size_t)(b + u * 32 < b1 ? b + u * 32 : b) * 8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (b + u * 32 < b1) sum += v[u];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) red[sl * 32 + e4 * 4 + u] = sum[u];
  __syncthreads();
  for (int half = 16; half >= 1; half >>= 1) {       // tree over the 32 slices
    for (int e = tid; e < half * 32; e += WG) red[e] += red[half * 32 + e];
    __syncthreads();
  }
  // the share goes out with device-scope (write-through) stores, the ticket is taken once they have
  // completed, and the last workgroup reads the shares with device-scope loads: no fence, which
  // costs 10 us on gfx950 even when the L2 holds nothing dirty
  if (tid < 32) __hip_atomic_store(scratch + bid * 32 + tid, red[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // (the ticket lives behind the shares of THIS call's scratch -- zero when the buffer is made, set back by the
  // last workgroup -- so that two solver objects, or two streams, never elect across each other's launches)
  unsigned* ticket = reinterpret_cast<unsigned*>(scratch + FIN32_WG * 32);
  if (tid == 0) s_last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == FIN32_WG - 1);
  __syncthreads();
  if (!s_last) return;
  {
    // eight shares per thread, all loads in flight at once (one after the other they cost 0.3 us each)
    const int e = tid & 31, g8 = tid >> 5;
    double v[FIN32_WG / 8];
#pragma unroll
    for (int u = 0; u < FIN32_WG / 8; ++u)
      v[u] = __hip_atomic_load(scratch + (g8 * (FIN32_WG / 8) + u) * 32 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double tot = 0.0;
#pragma unroll
    for (int u = 0; u < FIN32_WG / 8; ++u) tot += v[u];
    red[g8 * 32 + e] = tot;
  }
  __syncthreads();
  if (tid < 32) {
    double tot = red[tid];
#pragma unroll
    for (int g = 1; g < 8; ++g) tot += red[g * 32 + tid];
    out[tid] = tot;
  }
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t > 0) {
    __threadfence_block();
    __syncthreads();
    potrf_alpha_wg(out, t, T, mu, alpha, info, red, red + 256);
  }
  if (rtr) {      // the residual norm next to the block, as k_finish_trace (same order of additions as k_trace_finish)
    __syncthreads();
    trace_finish_wg(rtr, rtr_nblk, rtr_ts, rtr_nc, res2, info, nullptr, red);
  }
}
__global__ __launch_bounds__(WG) void k_finish32(const double* __restrict__ partials, int nblk,
                                                 double* scratch, int t, int T, double* out,
                                                 double* __restrict__ mu, double* __restrict__ alpha,
                                                 int* __restrict__ info, const double* __restrict__ rtr,
                                                 int rtr_nblk, int rtr_ts, int rtr_nc, double* __restrict__ res2) {
  __shared__ double red[32 * 32];
  __shared__ int s_last;
  finish32_wg(partials, nblk, scratch, t, T, out, mu, alpha, info, rtr, rtr_nblk, rtr_ts, rtr_nc, res2, blockIdx.x,
              red, s_last);
}
// Two k_finish32 in one launch (2 FIN32_WG workgroups): the first half sums the blocks the SpMM left, factors and
// forms alpha (t > 0); the second half sums the blocks the block solve left (beta).  Each half is one k_finish32 --
// same shares, same order of additions, own scratch and ticket -- so both results are those of two launches.
__global__ __launch_bounds__(WG) void k_finish32_pair(const double* __restrict__ pa, int na, double* sa, int t, int T,
                                                      double* outa, double* __restrict__ mu, double* __restrict__ alpha,
                                                      int* __restrict__ info, const double* __restrict__ pb, int nb,
                                                      double* sb, double* outb) {
  __shared__ double red[32 * 32];
  __shared__ int s_last;
  if (blockIdx.x < FIN32_WG)
    finish32_wg(pa, na, sa, t, T, outa, mu, alpha, info, nullptr, 0, 0, 0, nullptr, blockIdx.x, red, s_last);
  else
    finish32_wg(pb, nb, sb, 0, 0, outb, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, blockIdx.x - FIN32_WG,
                red, s_last);
}

// t x t upper Cholesky, one lane (t <= 16).  LAPACK dpotf2 'U': on failure
// the failing pivot is stored and the rest of W is left untouched.
__global__ void k_potrf(double* __restrict__ Wg, int t, int* __restrict__ info) {
  __shared__ double W[16 * 16];
  for (int e = threadIdx.x; e < t * t; e += 64) W[e] = Wg[e];
  __syncthreads();
  potrf_upper_wg(W, t, info);
  for (int e = threadIdx.x; e < t * t; e += 64) Wg[e] = W[e];
}

// Small t x t work of the fused Orthodir step (ecg.c:577-587), one lane:
// mu = U^T U ; beta <- beta U^-1 (bm x bn) ; alpha <- U^-T alpha (t x nrhs) ;
// beta(0:t, 0:t) <- U^-T beta(0:t, 0:t).
__global__ void k_fused_small(double* __restrict__ mu, int t, int nrhs, int bm, int bn, int ldb,
                              double* __restrict__ alpha, double* __restrict__ beta,
                              int* __restrict__ info) {
  if (threadIdx.x != 0) return;
  int fail = 0;
  for (int j = 0; j < t; ++j) {
    double d = mu[j + t * j];
    for (int k = 0; k < j; ++k) d -= mu[k + t * j] * mu[k + t * j];
    if (!(d > 0.0)) { mu[j + t * j] = d; fail = j + 1; break; }
    d = sqrt(d);
    mu[j + t * j] = d;
    for (int i = j + 1; i < t; ++i) {
      double s = mu[j + t * i];
      for (int k = 0; k < j; ++k) s -= mu[k + t * j] * mu[k + t * i];
      mu[j + t * i] = s / d;
    }
  }
  *info = fail;
  for (int j = 0; j < bn && j < t; ++j) {      // beta <- beta U^-1
    for (int k = 0; k < j; ++k) {
      const double u = mu[k + t * j];
      for (int i = 0; i < bm; ++i) beta[i + ldb * j] -= beta[i + ldb * k] * u;
    }
    const double d = 1.0 / mu[j + t * j];
    for (int i = 0; i < bm; ++i) beta[i + ldb * j] *= d;
  }
  for (int c = 0; c < nrhs; ++c)                 // alpha <- U^-T alpha
    for (int i = 0; i < t; ++i) {
      double s = alpha[i + t * c];
      for (int k = 0; k < i; ++k) s -= mu[k + t * i] * alpha[k + t * c];
      alpha[i + t * c] = s / mu[i + t * i];
    }
  for (int c = 0; c < t; ++c)                    // beta(0:t,0:t) <- U^-T beta(0:t,0:t)
    for (int i = 0; i < t; ++i) {
      double s = beta[i + ldb * c];
      for (int k = 0; k < i; ++k) s -= mu[k + t * i] * beta[k + ldb * c];
      beta[i + ldb * c] = s / mu[i + t * i];
    }
}

// -------------------------------------------------------------- updates ----
// P <- P U^-1 (and AP) by forward substitution along each row, one row/lane.
template <int TS>
__global__ __launch_bounds__(WG) void k_trsm(int m, int t, const double* __restrict__ U,
                                             double* __restrict__ P, double* __restrict__ AP) {
  __shared__ double su[TS * TS];
  __shared__ double sd[TS];
  for (int e = threadIdx.x; e < t * t; e += WG) su[e] = U[e];
  __syncthreads();
  if (threadIdx.x < t) sd[threadIdx.x] = 1.0 / su[threadIdx.x + t * threadIdx.x];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double p[TS];
    load_row<TS>(P, row, p);
#pragma unroll
    for (int j = 0; j < TS; ++j) {
      if (j < t) {
        double s = p[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = fma(-p[k], su[k + t * j], s);
        p[j] = s * sd[j];
      }
    }
    store_row<TS>(P, row, p);
    if (AP) {
      load_row<TS>(AP, row, p);
#pragma unroll
      for (int j = 0; j < TS; ++j) {
        if (j < t) {
          double s = p[j];
#pragma unroll
          for (int k = 0; k < j; ++k) s = fma(-p[k], su[k + t * j], s);
          p[j] = s * sd[j];
        }
      }
      store_row<TS>(AP, row, p);
    }
  }
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

// X += P alpha, R -= AP alpha, plus per-workgroup sums of R(:,c)^2.
template <int TS>
__global__ __launch_bounds__(WG) void k_update_xr(int m, int t, int nc,
                                                  const double* __restrict__ alpha,
                                                  const double* __restrict__ P,
                                                  const double* __restrict__ AP,
                                                  double* __restrict__ X, double* __restrict__ R,
                                                  double* __restrict__ rtr) {
  __shared__ double sa[TS * TS];
  for (int e = threadIdx.x; e < t * nc; e += WG) sa[e] = alpha[e];
  __syncthreads();
  double rr[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) rr[c] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double p[TS], ap[TS], x[TS], r[TS];
    load_row<TS>(P, row, p);
    load_row<TS>(AP, row, ap);
    load_row<TS>(X, row, x);
    load_row<TS>(R, row, r);
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      if (c < nc) {
        double sx = 0.0, sr = 0.0;
#pragma unroll
        for (int k = 0; k < TS; ++k) {
          if (k < t) {
            const double a = sa[k + t * c];
            sx = fma(p[k], a, sx);
            sr = fma(ap[k], a, sr);
          }
        }
        x[c] += sx;
        r[c] -= sr;
        rr[c] = fma(r[c], r[c], rr[c]);
      }
    }
    store_row<TS>(X, row, x);
    store_row<TS>(R, row, r);
  }
  block_sum_cols<TS>(rr, rtr + (size_t)blockIdx.x * TS);
}

__global__ void k_potrf_alpha(const double* __restrict__ buf, int t, int T, double* __restrict__ mu,
                              double* __restrict__ alpha, int* __restrict__ info) {
  __shared__ double W[16 * 16];
  __shared__ double G[16 * 16];
  potrf_alpha_wg(buf, t, T, mu, alpha, info, W, G);
}

// P <- P U^-1, AP <- AP U^-1, X += P alpha, R -= AP alpha and the column sums of
// R^2 in one pass over the four panels (ecg.c:434-435 + :500-501 + :250).
// gram != null (runs of several processes, where an all-reduce of [W ; G^T] sits between the Gram
// kernel and this one): every workgroup factors W and forms alpha itself (k_potrf_alpha's
// arithmetic, a microsecond), workgroup 0 stores them and the status -- one launch less.
// Prologue of k_trsm_update / k_update_xrz, whole workgroup: U (su), 1 / diag(U) (sd) and alpha (sa) into LDS -- from
// U and alpha, or formed from gram = [W ; G^T] -- and, ukeep != null, U kept there by workgroup 0.
template <int TS>
__device__ __forceinline__ void trsm_update_prologue(int t, int nc, double* U, double* alpha, const double* gram,
                                                     int* info, double* __restrict__ ukeep, double* su, double* sd,
                                                     double* sa) {
  if (gram) {
    const bool first = blockIdx.x == 0;
    potrf_alpha_wg(gram, t, nc, first ? U : nullptr, first ? alpha : nullptr, first ? info : nullptr, su, sa);
  } else {
    for (int e = threadIdx.x; e < t * t; e += WG) su[e] = U[e];
    for (int e = threadIdx.x; e < t * nc; e += WG) sa[e] = alpha[e];
  }
  __syncthreads();
  if (threadIdx.x < t) sd[threadIdx.x] = 1.0 / su[threadIdx.x + t * threadIdx.x];
  // ukeep (lazy normalisation, ecg.c): P and AP stay as they are -- the rows below are normalised in
  // registers for X and R only -- and the factor is kept for the kernels that meet the raw panels later
  if (ukeep && blockIdx.x == 0) for (int e = threadIdx.x; e < t * t; e += WG) ukeep[e] = su[e];
  __syncthreads();
}
// One row of k_trsm_update / k_update_xrz: p <- p U^-1, ap <- ap U^-1 (in registers), x += p alpha, r -= ap alpha,
// rr += r^2 per column.
template <int TS>
__device__ __forceinline__ void trsm_update_row(double (&p)[TS], double (&ap)[TS], double (&x)[TS], double (&r)[TS],
                                                double (&rr)[TS], const double* su, const double* sd, const double* sa,
                                                int t, int nc) {
#pragma unroll
  for (int j = 0; j < TS; ++j) {
    if (j < t) {
      double s1 = p[j], s2 = ap[j];
#pragma unroll
      for (int k = 0; k < j; ++k) { const double u = su[k + t * j]; s1 = fma(-p[k], u, s1); s2 = fma(-ap[k], u, s2); }
      p[j] = s1 * sd[j];
      ap[j] = s2 * sd[j];
    }
  }
#pragma unroll
  for (int c = 0; c < TS; ++c) {
    if (c < nc) {
      double sx = 0.0, sr = 0.0;
#pragma unroll
      for (int k = 0; k < TS; ++k) {
        if (k < t) {
          const double a = sa[k + t * c];
          sx = fma(p[k], a, sx);
          sr = fma(ap[k], a, sr);
        }
      }
      x[c] += sx;
      r[c] -= sr;
      rr[c] = fma(r[c], r[c], rr[c]);
    }
  }
}

template <int TS>
__global__ __launch_bounds__(WG) void k_trsm_update(int m, int t, int nc, double* U, double* alpha,
                                                    double* __restrict__ P, double* __restrict__ AP,
                                                    double* __restrict__ X, double* __restrict__ R,
                                                    double* __restrict__ rtr, const double* gram, int* info,
                                                    double* __restrict__ ukeep, int xnt) {
  __shared__ double su[TS * TS];
  __shared__ double sd[TS];
  __shared__ double sa[TS * TS];
  trsm_update_prologue<TS>(t, nc, U, alpha, gram, info, ukeep, su, sd, sa);
  double rr[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) rr[c] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double p[TS], ap[TS], x[TS], r[TS];
    load_row<TS>(P, row, p);
    load_row<TS>(AP, row, ap);
    // X is the one panel nobody reads again before the caches have turned over (its next reader is this kernel, an
    // iteration later): read and written with the nontemporal hint its 2 x 33 MB do not push R -- which the block
    // solve reads next -- out of the caches, nor wait there as dirty lines: the block solve behind this kernel
    // 125.5 -> 121.0 us, this kernel +0.5 us (six alternations in one box, profiles/r04_nontemporal_x_ab.txt).  The
    // hint on the store alone or on the load alone does nothing; on the loads of P / AP, or of P / P_prev in
    // k_update_z, it costs 2-5 us; on the X accesses of k_trsm_update_mfma<8 / 16> it changes nothing.
    // xnt = 0 (the launcher: a panel below 16 MiB, e.g. one GPU's share of a small problem): X stays in the
    // caches from one iteration to the next and the hint would send it to memory
    if (xnt) load_row_nt<TS>(X, row, x); else load_row<TS>(X, row, x);
    load_row<TS>(R, row, r);
    trsm_update_row<TS>(p, ap, x, r, rr, su, sd, sa, t, nc);
    if (!ukeep) {
      store_row<TS>(P, row, p);
      store_row<TS>(AP, row, ap);
    }
    if (xnt) store_row_nt<TS>(X, row, x); else store_row<TS>(X, row, x);
    store_row<TS>(R, row, r);
  }
  block_sum_cols<TS>(rr, rtr + (size_t)blockIdx.x * TS);
}

// The same pass for panels of 8 and 16 columns on the f64 matrix cores.  With Ui = U^-1 (formed
// once per workgroup, t <= 16) and B = Ui alpha, all four results are products of the OLD tiles:
//   P <- P Ui,  AP <- AP Ui,  X += P B,  R -= AP B,
// so a tile of 16 rows of P / AP is loaded once in the A layout of v_mfma_f64_16x16x4 (lane l:
// row l&15, k = 4s + (l>>4)) and multiplied by per-lane constants (B layout: k = 4s + (l>>4),
// column l&15); X and R pass through the accumulator (C/D layout: four coalesced 512-byte rows).
// Columns beyond t ride along unchanged (Ui is padded with the identity, B with zeros).
// TS = 16: one tile per panel.  TS = 8: [P | AP] is one 16-wide A operand, blockdiag(Ui, Ui) and
// [B 0; 0 -B] the B operands, [X | R] the accumulator.
template <int TS>
__global__ __launch_bounds__(WG) void k_trsm_update_mfma(int m, int t, int nc, double* Ug, double* alphag,
                                                         double* __restrict__ P, double* __restrict__ AP,
                                                         double* __restrict__ X, double* __restrict__ R,
                                                         double* __restrict__ rtr, const double* gram, int* info,
                                                         double* __restrict__ ukeep) {
  static_assert(TS == 8 || TS == 16, "matrix-core variant: panels of 8 or 16 columns");
  __shared__ double su[16 * 16];    // U (column major, leading dimension 16, identity beyond t)
  __shared__ double si[16 * 16];    // Ui = U^-1
  __shared__ double sb[16 * 16];    // B = Ui alpha (16 x 16, zero beyond t x nc)
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lo = lane & 15, hi = lane >> 4;
  __shared__ double sw[16 * 16];    // gram != null: U and alpha as this workgroup computes them (k_trsm_update)
  __shared__ double sg[16 * 16];
  const double* U = Ug;
  const double* alpha = alphag;
  if (gram) {
    const bool first = blockIdx.x == 0;
    potrf_alpha_wg(gram, t, nc, first ? Ug : nullptr, first ? alphag : nullptr, first ? info : nullptr, sw, sg);
    __syncthreads();
    U = sw; alpha = sg;
  }
  for (int e = tid; e < 256; e += WG) {
    const int i = e & 15, j = e >> 4;
    su[e] = (i < t && j < t) ? U[i + t * j] : (i == j ? 1.0 : 0.0);
    sb[e] = 0.0;
  }
  // ukeep (lazy normalisation): P and AP are left as they are, the factor is kept for pa_k_update_z
  if (ukeep && blockIdx.x == 0) for (int e = tid; e < t * t; e += WG) ukeep[e] = U[e];
  __syncthreads();
  if (tid < 16) {
    // column tid of Ui by back substitution: U x = e_tid (upper triangular)
    double x[16];
#pragma unroll
    for (int i = 15; i >= 0; --i) {
      double sv = (i == tid) ? 1.0 : 0.0;
#pragma unroll
      for (int k = i + 1; k < 16; ++k) sv -= su[i + 16 * k] * x[k];
      x[i] = sv / su[i + 16 * i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) si[i + 16 * tid] = x[i];
  }
  __syncthreads();
  for (int e = tid; e < 256; e += WG) {
    const int i = e & 15, c = e >> 4;
    double sv = 0.0;
    if (i < t && c < nc) for (int k = i; k < t; ++k) sv += si[i + 16 * k] * alpha[k + t * c];
    sb[e] = sv;
  }
  __syncthreads();
  // per-lane B operands: k = 4 s + hi
  double bu[4], bb[4];
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    const int k = 4 * s2 + hi;
    if (TS == 16) { bu[s2] = si[k + 16 * lo]; bb[s2] = sb[k + 16 * lo]; }
    else {
      // blockdiag(Ui, Ui): rows / columns 0..7 act on P, 8..15 on AP;  [B 0; 0 -B]
      const int kk = k & 7, cc = lo & 7;
      const bool same = (k < 8) == (lo < 8);
      bu[s2] = same ? si[kk + 16 * cc] : 0.0;
      bb[s2] = same ? (k < 8 ? sb[kk + 16 * cc] : -sb[kk + 16 * cc]) : 0.0;
    }
  }
  double rr = 0.0;   // sum of squares of the new R in column lo (TS = 8: lo - 8)
  const size_t ntile = ((size_t)m + 15) >> 4;
  const size_t tstride = (size_t)gridDim.x * (WG / 64);
  for (size_t tl = (size_t)blockIdx.x * (WG / 64) + wave; tl < ntile; tl += tstride) {
    const size_t r0 = tl << 4;
    const size_t arow = r0 + lo;
    const bool aok = arow < (size_t)m;
    if (TS == 16) {
      double ap_[4], aap[4];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
        ap_[s2] = aok ? P[arow * 16 + 4 * s2 + hi] : 0.0;
        aap[s2] = aok ? AP[arow * 16 + 4 * s2 + hi] : 0.0;
      }
      mfma_d4 x, r, pn = mfma_d4{0.0, 0.0, 0.0, 0.0}, apn = mfma_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t row = r0 + hi + 4 * q;
        const bool ok = row < (size_t)m;
        x[q] = ok ? X[row * 16 + lo] : 0.0;
        r[q] = ok ? R[row * 16 + lo] : 0.0;
      }
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
        if (!ukeep) {
          pn = __builtin_amdgcn_mfma_f64_16x16x4f64(ap_[s2], bu[s2], pn, 0, 0, 0);
          apn = __builtin_amdgcn_mfma_f64_16x16x4f64(aap[s2], bu[s2], apn, 0, 0, 0);
        }
        x = __builtin_amdgcn_mfma_f64_16x16x4f64(ap_[s2], bb[s2], x, 0, 0, 0);
        r = __builtin_amdgcn_mfma_f64_16x16x4f64(aap[s2], -bb[s2], r, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t row = r0 + hi + 4 * q;
        if (row < (size_t)m) {
          if (!ukeep) { P[row * 16 + lo] = pn[q]; AP[row * 16 + lo] = apn[q]; }
          X[row * 16 + lo] = x[q]; R[row * 16 + lo] = r[q];
          if (lo < nc) rr = fma(r[q], r[q], rr);
        }
      }
    } else {
      double a[4];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
        const int k = 4 * s2 + hi;
        a[s2] = aok ? (k < 8 ? P[arow * 8 + k] : AP[arow * 8 + k - 8]) : 0.0;
      }
      mfma_d4 xr, pn = mfma_d4{0.0, 0.0, 0.0, 0.0};
      double* __restrict__ XR = lo < 8 ? X : R;
      double* __restrict__ PA = lo < 8 ? P : AP;
      const int cc = lo & 7;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t row = r0 + hi + 4 * q;
        xr[q] = row < (size_t)m ? XR[row * 8 + cc] : 0.0;
      }
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
        if (!ukeep) pn = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], bu[s2], pn, 0, 0, 0);
        xr = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], bb[s2], xr, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t row = r0 + hi + 4 * q;
        if (row < (size_t)m) {
          if (!ukeep) PA[row * 8 + cc] = pn[q];
          XR[row * 8 + cc] = xr[q];
          if (lo >= 8 && cc < nc) rr = fma(xr[q], xr[q], rr);
        }
      }
    }
  }
  // column sums of R^2: lanes with the same column (4 per wave), then the waves
  __shared__ double red[WG / 64][TS];
  rr += __shfl_xor(rr, 16);
  rr += __shfl_xor(rr, 32);
  if (TS == 16) { if (hi == 0) red[wave][lo] = rr; }
  else if (hi == 0 && lo >= 8) red[wave][lo - 8] = rr;
  __syncthreads();
  if (tid < TS) {
    double sv = red[0][tid];
#pragma unroll
    for (int w2 = 1; w2 < WG / 64; ++w2) sv += red[w2][tid];
    rtr[(size_t)blockIdx.x * TS + tid] = sv;
  }
}

template <int TS>
__global__ __launch_bounds__(WG) void k_colnorm2(int m, const double* __restrict__ R,
                                                 double* __restrict__ rtr) {
  double rr[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) rr[c] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double r[TS];
    load_row<TS>(R, row, r);
#pragma unroll
    for (int c = 0; c < TS; ++c) rr[c] = fma(r[c], r[c], rr[c]);
  }
  block_sum_cols<TS>(rr, rtr + (size_t)blockIdx.x * TS);
}

__global__ __launch_bounds__(WG) void k_trace_finish(const double* __restrict__ rtr, int nblk,
                                                     int ts, int nc, double* __restrict__ res2,
                                                     const int* __restrict__ info, double* host, double seq) {
  __shared__ double red[WG];
  trace_finish_wg(rtr, nblk, ts, nc, res2, info, host, red, seq);
}

// Lazy normalisation, panels of up to 4 columns (k_update_z<TS>, k_update_xrz): C0 = Ui, C1 = Ui (Ui^T G1 Ui),
// C2 = Up (Up^T G2 Ui) from the raw Gram blocks sb = [G1 ; G2] ((a_lo + a_hi) x a_lo) and the two factors sfac =
// [ucur | uprev] in LDS, into sc + 4, 5, 6 TS^2 (sc: 7 TS^2 doubles); called by a whole workgroup, ends synchronised.
template <int TS>
__device__ __forceinline__ void lazy_coeffs_wg(const double* sb, const double* sfac, int a_lo, int a_hi, double* sc) {
  const int na = a_lo + a_hi;
  const int t = a_lo, tt = t * t, tid = threadIdx.x;
  double* Ui = sc; double* Up = sc + TS * TS; double* T1 = sc + 2 * TS * TS; double* T2 = sc + 3 * TS * TS;
  double* C0 = sc + 4 * TS * TS; double* C1 = sc + 5 * TS * TS; double* C2 = sc + 6 * TS * TS;
  if (tid < 64) {
    if (tid < 2 * t) {          // column c of the inverse of an upper-triangular factor: back substitution on e_c
      const double* Uf = tid < t ? sfac : sfac + tt;
      double* inv = tid < t ? Ui : Up;
      const int c = tid < t ? tid : tid - t;
      double x[TS];
#pragma unroll
      for (int i = TS - 1; i >= 0; --i) {
        x[i] = 0.0;
        if (i < t && i <= c) {
          double sv = i == c ? 1.0 : 0.0;
#pragma unroll
          for (int k = i + 1; k < TS; ++k) if (k < t && k <= c) sv = fma(-Uf[i + t * k], x[k], sv);
          x[i] = sv / Uf[i + t * i];
        }
      }
#pragma unroll
      for (int i = 0; i < TS; ++i) if (i < t) inv[i + t * c] = x[i];
    }
    wave_lds_sync();
    const int r = tid % (t > 0 ? t : 1), c = tid / (t > 0 ? t : 1);
    const bool on = tid < tt;
    if (on) {                     // T1 = G1 Ui, T2 = G2 Ui
      double s1 = 0.0, s2 = 0.0;
      for (int k = 0; k < t; ++k) { s1 = fma(sb[r + na * k], Ui[k + t * c], s1); if (a_hi > 0) s2 = fma(sb[a_lo + r + na * k], Ui[k + t * c], s2); }
      T1[tid] = s1; T2[tid] = s2;
    }
    wave_lds_sync();
    double b1 = 0.0, b2 = 0.0;
    if (on) {                     // beta1 = Ui^T T1, beta2 = Up^T T2
      for (int k = 0; k < t; ++k) { b1 = fma(Ui[k + t * r], T1[k + t * c], b1); b2 = fma(Up[k + t * r], T2[k + t * c], b2); }
    }
    wave_lds_sync();
    if (on) { T1[tid] = b1; T2[tid] = b2; }
    wave_lds_sync();
    if (on) {                     // C1 = Ui beta1, C2 = Up beta2, C0 = Ui
      double c1 = 0.0, c2 = 0.0;
      for (int k = 0; k < t; ++k) { c1 = fma(Ui[r + t * k], T1[k + t * c], c1); c2 = fma(Up[r + t * k], T2[k + t * c], c2); }
      C0[tid] = Ui[tid]; C1[tid] = c1; C2[tid] = c2;
    }
  }
  __syncthreads();
}
// One row of Z: o = z C0 - v0 C1 - v1 C2 on the first nc columns, z elsewhere.
template <int TS>
__device__ __forceinline__ void update_z_lazy_row(const double (&z)[TS], const double (&v0)[TS], const double (&v1)[TS],
                                                  double (&o)[TS], const double* C0, const double* C1, const double* C2,
                                                  int t, int a_hi, int nc) {
#pragma unroll
  for (int c = 0; c < TS; ++c) {
    o[c] = z[c];
    if (c < nc) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < TS; ++k)
        if (k < t) { s = fma(z[k], C0[k + t * c], s); s = fma(-v0[k], C1[k + t * c], s); if (a_hi > 0) s = fma(-v1[k], C2[k + t * c], s); }
      o[c] = s;
    }
  }
}

// Z(:, :nc) -= [V0(:, :a_lo) | V1(:, :a_hi)] beta
template <int TS>
__global__ __launch_bounds__(WG) void k_update_z(int m, int a_lo, int a_hi, int nc,
                                                 const double* __restrict__ beta, int ldb,
                                                 const double* __restrict__ V0,
                                                 const double* __restrict__ V1,
                                                 double* __restrict__ Z,
    const double* note_src, double* note_host, double note_seq,
    const double* __restrict__ ucur, const double* __restrict__ uprev,
    const int* __restrict__ pk_off, const int* __restrict__ pk_slot, double* __restrict__ sendbuf) {
  // pk_off != null (several processes, pa_k_update_z_pack): the new rows of Z are the next product's X -- the rows
  // the neighbours need go into the send buffer from here (row r into the slots pk_slot[pk_off[r] .. pk_off[r + 1])),
  // k_pack_rows is not launched
  __shared__ double sb[2 * TS * TS];
  __shared__ double sc[7 * TS * TS];
  // (note_host: two words the host is waiting for -- the all-reduced residual norm and the
  // factorisation status next to beta -- go out to pinned memory from here: no copy, no extra launch)
  if (note_host && blockIdx.x == 0 && threadIdx.x == 0) {
    __hip_atomic_store(note_host, note_src[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(note_host + 1, note_src[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    if (note_seq != 0.0) __hip_atomic_store(note_host + 2, note_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const int na = a_lo + a_hi;
  for (int e = threadIdx.x; e < na * nc; e += WG) sb[e] = beta[(e % na) + ldb * (e / na)];
  // (lazy normalisation: the two factors come in with the same round trip as beta -- read from memory inside
  // the back substitution below, behind run-time conditions, they cost several trips in a row at the head of
  // every workgroup)
  __shared__ double sfac[2 * TS * TS];
  if (ucur) {
    const int tt0 = a_lo * a_lo;
    for (int e = threadIdx.x; e < 2 * tt0; e += WG) sfac[e] = e < tt0 ? ucur[e] : (uprev ? uprev[e - tt0] : 0.0);
  }
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  if (ucur) {
    // Lazy normalisation (ecg.c: Orthodir without block-size reduction, panels of up to 4 columns): the panels
    // were never multiplied by U^-1 -- V0 = P_raw and Z = M^-1 AP_raw belong to the factor U = ucur of this
    // iteration, V1 = P_prev_raw to uprev -- and `beta` holds the RAW Gram blocks G1 = AP_raw^T Z_raw, G2 =
    // AP_prev_raw^T Z_raw.  With Ui = U^-1, Up = uprev^-1 the reference's update Z_n - P_n beta1 - P_prev_n beta2
    // (ecg.c:510-517 on the normalised panels) is  Z_raw C0 - P_raw C1 - P_prev_raw C2,  C0 = Ui,
    // C1 = Ui (Ui^T G1 Ui), C2 = Up (Up^T G2 Ui): sixteen threads form the three t x t blocks in LDS.
    lazy_coeffs_wg<TS>(sb, sfac, a_lo, a_hi, sc);
    const double* C0 = sc + 4 * TS * TS; const double* C1 = sc + 5 * TS * TS; const double* C2 = sc + 6 * TS * TS;
    const int t = a_lo;
    for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
      double z[TS], v0[TS], v1[TS], o[TS];
      load_row<TS>(Z, row, z);
      load_row<TS>(V0, row, v0);
      if (a_hi > 0) load_row<TS>(V1, row, v1);
      update_z_lazy_row<TS>(z, v0, v1, o, C0, C1, C2, t, a_hi, nc);
      store_row<TS>(Z, row, o);
      if (pk_off) for (int k = pk_off[row], k1 = pk_off[row + 1]; k < k1; ++k) store_row<TS>(sendbuf, (size_t)pk_slot[k], o);
    }
    return;
  }
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double z[TS], v0[TS], v1[TS];
    load_row<TS>(Z, row, z);
    load_row<TS>(V0, row, v0);
    if (a_hi > 0) load_row<TS>(V1, row, v1);
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      if (c < nc) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < TS; ++k)
          if (k < a_lo) s = fma(v0[k], sb[k + na * c], s);
        if (a_hi > 0) {
#pragma unroll
          for (int k = 0; k < TS; ++k)
            if (k < a_hi) s = fma(v1[k], sb[a_lo + k + na * c], s);
        }
        z[c] -= s;
      }
    }
    store_row<TS>(Z, row, z);
    if (pk_off) for (int k = pk_off[row], k1 = pk_off[row + 1]; k < k1; ++k) store_row<TS>(sendbuf, (size_t)pk_slot[k], z);
  }
}

// k_trsm_update (lazy normalisation: ukeep, X nontemporal under xnt) and k_update_z (lazy coefficients, V0 = P,
// V1 = P_prev, a_lo = a_hi = nc = t) in one pass over the rows, for the order in which the block solve runs before
// the update (ecg.c: solve_first): both halves of the update read P, so P is read once, and the six panels go
// through one launch.  Per element the arithmetic of the two kernels (the same device functions); the grid, the
// row -> workgroup map and the column sums of R^2 are k_trsm_update's (update_grid), so k_trace_finish forms the
// same norm.  ucur of k_update_z is U itself: the factor k_trsm_update keeps in ukeep for it.
template <int TS>
__global__ __launch_bounds__(WG) void k_update_xrz(int m, int t, double* U, double* alpha, const double* __restrict__ P,
                                                   const double* __restrict__ AP, const double* __restrict__ Pprev,
                                                   double* __restrict__ X, double* __restrict__ R,
                                                   double* __restrict__ Z, double* __restrict__ rtr,
                                                   double* __restrict__ ukeep, const double* __restrict__ beta,
                                                   int ldb, const double* __restrict__ uprev, int xnt) {
  __shared__ double su[TS * TS];
  __shared__ double sd[TS];
  __shared__ double sa[TS * TS];
  __shared__ double sb[2 * TS * TS];
  __shared__ double sfac[2 * TS * TS];
  __shared__ double sc[7 * TS * TS];
  const int na = 2 * t, tt = t * t;
  for (int e = threadIdx.x; e < na * t; e += WG) sb[e] = beta[(e % na) + ldb * (e / na)];
  for (int e = threadIdx.x; e < 2 * tt; e += WG) sfac[e] = e < tt ? U[e] : uprev[e - tt];
  trsm_update_prologue<TS>(t, t, U, alpha, nullptr, nullptr, ukeep, su, sd, sa);    // (its barriers cover sb / sfac)
  lazy_coeffs_wg<TS>(sb, sfac, t, t, sc);
  const double* C0 = sc + 4 * TS * TS; const double* C1 = sc + 5 * TS * TS; const double* C2 = sc + 6 * TS * TS;
  double rr[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) rr[c] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double p[TS], ap[TS], x[TS], r[TS], z[TS], v0[TS], v1[TS], o[TS];
    load_row<TS>(P, row, v0);
    load_row<TS>(AP, row, ap);
    if (xnt) load_row_nt<TS>(X, row, x); else load_row<TS>(X, row, x);
    load_row<TS>(R, row, r);
    load_row<TS>(Z, row, z);
    load_row<TS>(Pprev, row, v1);
#pragma unroll
    for (int c = 0; c < TS; ++c) p[c] = v0[c];      // (normalised in registers below; Z's update takes the raw row)
    trsm_update_row<TS>(p, ap, x, r, rr, su, sd, sa, t, t);
    update_z_lazy_row<TS>(z, v0, v1, o, C0, C1, C2, t, t, t);
    if (xnt) store_row_nt<TS>(X, row, x); else store_row<TS>(X, row, x);
    store_row<TS>(R, row, r);
    store_row<TS>(Z, row, o);
  }
  block_sum_cols<TS>(rr, rtr + (size_t)blockIdx.x * TS);
}

// 16-column panels on the f64 matrix cores: a tile of 16 rows of Z is the C/D operand (lane l
// holds Z[row (l>>4) + 4r][col l&15]: four fully coalesced 512-byte accesses), the rows of
// [V0 | V1] are the A operand (A[row l&15][k = 4s + (l>>4)], 32-byte pieces of 16 rows per
// load, every cache line used up over four loads) and -beta the B operand, a per-lane constant.
// Lazy normalisation, panels of 8 / 16 columns (see k_update_z<TS>): C0 = Ui, C1 = Ui (Ui^T G1 Ui), C2 = Up (Up^T G2 Ui)
// from the raw Gram blocks in `beta` and the two kept factors, as 16 x 16 blocks (leading dimension 16, zero
// beyond t) in LDS; called by a whole workgroup of WG threads.  sc = 7 * 256 doubles.
__device__ __forceinline__ void lazy_coeffs16(const double* __restrict__ beta, int ldb, int t, int a_hi,
                                              const double* __restrict__ ucur, const double* __restrict__ uprev,
                                              double* sc) {
  double* Ui = sc; double* Up = sc + 256; double* T1 = sc + 512; double* T2 = sc + 768;
  double* C0 = sc + 1024; double* C1 = sc + 1280; double* C2 = sc + 1536;
  const int tid = threadIdx.x;
  for (int e = tid; e < 256; e += WG) {       // the factors, identity beyond t (T1 / T2 serve as staging)
    const int i = e & 15, j = e >> 4;
    T1[e] = (i < t && j < t) ? ucur[i + t * j] : (i == j ? 1.0 : 0.0);
    T2[e] = (i < t && j < t) ? uprev[i + t * j] : (i == j ? 1.0 : 0.0);
    // the raw Gram blocks with the same round trip (C1 / C2 serve as staging until they are written at the end):
    // read from memory inside the loop over k below they cost t trips in a row at the head of every workgroup
    C1[e] = (i < t && j < t) ? beta[i + ldb * j] : 0.0;
    C2[e] = (a_hi > 0 && i < t && j < t) ? beta[t + i + ldb * j] : 0.0;
  }
  __syncthreads();
  if (tid < 32) {                             // column c of an inverse by back substitution on e_c
    const double* Uf = tid < 16 ? T1 : T2;
    double* inv = tid < 16 ? Ui : Up;
    const int c = tid & 15;
    double x[16];
#pragma unroll
    for (int i = 15; i >= 0; --i) {
      double sv = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = i + 1; k < 16; ++k) sv -= Uf[i + 16 * k] * x[k];
      x[i] = sv / Uf[i + 16 * i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) inv[i + 16 * c] = x[i];
  }
  __syncthreads();
  const int r = tid & 15, c = tid >> 4;       // WG = 256: one entry each
  const bool on = r < t && c < t;
  {
    double s1 = 0.0, s2 = 0.0;                // T = G Ui
    if (on) for (int k = 0; k < t; ++k) {
      s1 = fma(C1[r + 16 * k], Ui[k + 16 * c], s1);
      if (a_hi > 0) s2 = fma(C2[r + 16 * k], Ui[k + 16 * c], s2);
    }
    __syncthreads();
    T1[tid] = s1; T2[tid] = s2;
  }
  __syncthreads();
  double b1 = 0.0, b2 = 0.0;                  // beta1 = Ui^T T1, beta2 = Up^T T2
  if (on) for (int k = 0; k < t; ++k) { b1 = fma(Ui[k + 16 * r], T1[k + 16 * c], b1); b2 = fma(Up[k + 16 * r], T2[k + 16 * c], b2); }
  __syncthreads();
  T1[tid] = b1; T2[tid] = b2;
  __syncthreads();
  double c1 = 0.0, c2 = 0.0;                  // C1 = Ui beta1, C2 = Up beta2
  if (on) for (int k = 0; k < t; ++k) { c1 = fma(Ui[r + 16 * k], T1[k + 16 * c], c1); c2 = fma(Up[r + 16 * k], T2[k + 16 * c], c2); }
  C0[tid] = on ? Ui[tid] : 0.0; C1[tid] = c1; C2[tid] = c2;
  __syncthreads();
}

// Z^T Z next to the update (BF-Omin forms it right behind, ecg.c:361 of the reference: G = P^T P with P = Z): a
// tile of the new Z in the accumulator layout -- lane (lo, hi): row hi + 4 r, column lo -- is the A operand AND the
// B operand of step r as it stands (A[i = lo][k = hi], B[k = hi][j = lo], k = the row), so the product costs four
// matrix instructions per tile and no data movement.  zzc = columns that count (the rest of a 16-wide tile is 0).
__device__ __forceinline__ void update_z_gram_step(const mfma_d4& z, mfma_d4& zz, size_t r0, int hi, int lo, int m, int zzc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double zm = (r0 + hi + 4 * r < (size_t)m && lo < zzc) ? z[r] : 0.0;
    zz = __builtin_amdgcn_mfma_f64_16x16x4f64(zm, zm, zz, 0, 0, 0);
  }
}
// the four wavefronts' sums -> one TS x TS block per workgroup (column major, the layout of k_gram's partial blocks)
template <int TS>
__device__ __forceinline__ void update_z_gram_out(const mfma_d4& zz, double* sc, double* __restrict__ zzp, int wave, int lane) {
  __syncthreads();                       // (sc may still hold the coefficient blocks of the prologue)
#pragma unroll
  for (int r = 0; r < 4; ++r) sc[wave * 256 + r * 64 + lane] = zz[r];
  __syncthreads();
  const int tid = threadIdx.x;           // WG = 256: entry (r, lane) of the tile each
  const int r = tid >> 6, l = tid & 63, i = (l >> 4) + 4 * r, j = l & 15;
  double sm = sc[tid];
#pragma unroll
  for (int w = 1; w < WG / 64; ++w) sm += sc[w * 256 + tid];
  if (i < TS && j < TS) zzp[(size_t)blockIdx.x * TS * TS + i + TS * j] = sm;
}

__global__ __launch_bounds__(WG, 4) void k_update_z_mfma16(int m, int a_lo, int a_hi, int nc,
                                                        const double* __restrict__ beta, int ldb,
                                                        const double* __restrict__ V0,
                                                        const double* __restrict__ V1,
                                                        double* __restrict__ Z,
    const double* note_src, double* note_host, double note_seq,
    const double* __restrict__ ucur, const double* __restrict__ uprev, double* __restrict__ zzp, int zzc) {
  constexpr int TS = 16;
  __shared__ double sc[7 * 256];
  // (note_host: two words the host is waiting for -- the all-reduced residual norm and the
  // factorisation status next to beta -- go out to pinned memory from here: no copy, no extra launch)
  if (note_host && blockIdx.x == 0 && threadIdx.x == 0) {
    __hip_atomic_store(note_host, note_src[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(note_host + 1, note_src[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    if (note_seq != 0.0) __hip_atomic_store(note_host + 2, note_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lo = lane & 15, hi = lane >> 4;
  // B[k][j] = -beta(k, j), k = 4s + hi (s < 4: rows of beta that meet V0, s >= 4: V1), j = lo
  double bneg[8];
#pragma unroll
  for (int s2 = 0; s2 < 8; ++s2) {
    const int k = 4 * (s2 & 3) + hi;
    const bool first = s2 < 4;
    const bool ok = lo < nc && (first ? k < a_lo : k < a_hi);
    bneg[s2] = ok ? -beta[(first ? k : a_lo + k) + ldb * lo] : 0.0;
  }
  const size_t ntile = ((size_t)m + 15) >> 4;
  const size_t tstride = (size_t)gridDim.x * (WG / 64);
  if (ucur) {
    // lazy normalisation: Z <- Z C0 - V0 C1 - V1 C2 (k_update_z<TS>); Z is an A operand like the other two.
    // The k index of a matrix-core step is free as long as both operands agree on it: step s2 of lane (lo, hi)
    // takes k = 8 (s2 >> 1) + 2 hi + (s2 & 1), so that the lane's four entries of a row are two 16-byte loads and
    // the four lanes of a row read 64 contiguous bytes per load (k = 4 s2 + hi, one double per load and 32 B
    // between the lanes of a row, touched 16 lines a quarter each per load: 129 us against 94 us for the in-place
    // form at 16 columns; whole rows turned through a padded LDS tile per wavefront: 193 us).  The first tile is
    // requested in front of the coefficient prologue (a 16 x 16 inverse and three products per workgroup), every
    // further one in front of the stores of the tile before it.
    const double* __restrict__ V1p = a_hi > 0 ? V1 : V0;       // (no second panel: its coefficients are zero)
    lazy_coeffs16(beta, ldb, a_lo, a_hi, ucur, uprev, sc);
    double b0[4], b1[4], b2[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const int k = 8 * (s2 >> 1) + 2 * hi + (s2 & 1);
      b0[s2] = sc[1024 + k + 16 * lo]; b1[s2] = -sc[1280 + k + 16 * lo]; b2[s2] = a_hi > 0 ? -sc[1536 + k + 16 * lo] : 0.0;
    }
    double2 rg[6];
    size_t t = (size_t)blockIdx.x * (WG / 64) + wave;
    {
      const size_t tl = t < ntile ? t : ntile - 1, arow = (tl << 4) + lo;
      const size_t base = (arow < (size_t)m ? arow : 0) * TS + 2 * hi;
      rg[0] = *reinterpret_cast<const double2*>(Z + base); rg[1] = *reinterpret_cast<const double2*>(Z + base + 8);
      rg[2] = *reinterpret_cast<const double2*>(V0 + base); rg[3] = *reinterpret_cast<const double2*>(V0 + base + 8);
      rg[4] = *reinterpret_cast<const double2*>(V1p + base); rg[5] = *reinterpret_cast<const double2*>(V1p + base + 8);
    }
    while (t < ntile) {
      const size_t r0 = t << 4;
      const bool aok = r0 + lo < (size_t)m;
      const double az[4] = {aok ? rg[0].x : 0.0, aok ? rg[0].y : 0.0, aok ? rg[1].x : 0.0, aok ? rg[1].y : 0.0};
      const double a0[4] = {aok ? rg[2].x : 0.0, aok ? rg[2].y : 0.0, aok ? rg[3].x : 0.0, aok ? rg[3].y : 0.0};
      const double a1[4] = {aok ? rg[4].x : 0.0, aok ? rg[4].y : 0.0, aok ? rg[5].x : 0.0, aok ? rg[5].y : 0.0};
      mfma_d4 z = mfma_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
        z = __builtin_amdgcn_mfma_f64_16x16x4f64(az[s2], b0[s2], z, 0, 0, 0);
        z = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s2], b1[s2], z, 0, 0, 0);
        z = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s2], b2[s2], z, 0, 0, 0);
      }
      const size_t tn = t + tstride;
      {
        // the next tile's rows (the last round asks for its own tile once more: no branch around a load)
        const size_t tl = tn < ntile ? tn : t, arow = (tl << 4) + lo;
        const size_t base = (arow < (size_t)m ? arow : 0) * TS + 2 * hi;
        rg[0] = *reinterpret_cast<const double2*>(Z + base); rg[1] = *reinterpret_cast<const double2*>(Z + base + 8);
        rg[2] = *reinterpret_cast<const double2*>(V0 + base); rg[3] = *reinterpret_cast<const double2*>(V0 + base + 8);
        rg[4] = *reinterpret_cast<const double2*>(V1p + base); rg[5] = *reinterpret_cast<const double2*>(V1p + base + 8);
      }
      asm volatile("" ::: "memory");     // (every lane of the tile has read its rows of Z before any is overwritten)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t row = r0 + hi + 4 * r;
        if (row < (size_t)m && lo < nc) Z[row * TS + lo] = z[r];
      }
      t = tn;
    }
    return;
  }
  mfma_d4 zz = mfma_d4{0.0, 0.0, 0.0, 0.0};
  for (size_t t = (size_t)blockIdx.x * (WG / 64) + wave; t < ntile; t += tstride) {
    const size_t r0 = t << 4;
    mfma_d4 z;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t row = r0 + hi + 4 * r;
      z[r] = row < (size_t)m ? Z[row * TS + lo] : 0.0;
    }
    const size_t arow = r0 + lo;
    const bool aok = arow < (size_t)m;
    double a[8];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) a[s2] = aok ? V0[arow * TS + 4 * s2 + hi] : 0.0;
    if (a_hi > 0) {
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) a[4 + s2] = aok ? V1[arow * TS + 4 * s2 + hi] : 0.0;
    }
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) z = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], bneg[s2], z, 0, 0, 0);
    if (a_hi > 0) {
#pragma unroll
      for (int s2 = 4; s2 < 8; ++s2) z = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], bneg[s2], z, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t row = r0 + hi + 4 * r;
      if (row < (size_t)m && lo < nc) Z[row * TS + lo] = z[r];
    }
    if (zzp) update_z_gram_step(z, zz, r0, hi, lo, m, zzc);
  }
  if (zzp) update_z_gram_out<TS>(zz, sc, zzp, wave, lane);
}

// 8-column panels: [V0 | V1] is one 16-wide A operand (four k-steps), Z uses half the tile.
__global__ __launch_bounds__(WG) void k_update_z_mfma8(int m, int a_lo, int a_hi, int nc,
                                                       const double* __restrict__ beta, int ldb,
                                                       const double* __restrict__ V0,
                                                       const double* __restrict__ V1,
                                                       double* __restrict__ Z,
    const double* note_src, double* note_host, double note_seq,
    const double* __restrict__ ucur, const double* __restrict__ uprev, double* __restrict__ zzp, int zzc) {
  constexpr int TS = 8;
  __shared__ double sc[7 * 256];
  // (note_host: two words the host is waiting for -- the all-reduced residual norm and the
  // factorisation status next to beta -- go out to pinned memory from here: no copy, no extra launch)
  if (note_host && blockIdx.x == 0 && threadIdx.x == 0) {
    __hip_atomic_store(note_host, note_src[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(note_host + 1, note_src[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    if (note_seq != 0.0) __hip_atomic_store(note_host + 2, note_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lo = lane & 15, hi = lane >> 4;
  double bneg[4];
  bool von[4];
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    const int k = 4 * s2 + hi;                 // column of [V0 | V1]
    const bool first = k < TS;
    const int kk = first ? k : k - TS;
    von[s2] = first ? kk < a_lo : kk < a_hi;
    bneg[s2] = (von[s2] && lo < nc) ? -beta[(first ? kk : a_lo + kk) + ldb * lo] : 0.0;
  }
  const size_t ntile = ((size_t)m + 15) >> 4;
  const size_t tstride = (size_t)gridDim.x * (WG / 64);
  if (ucur) {
    // lazy normalisation: Z <- [V0 | V1 | Z] [-C1 ; -C2 ; C0], 24 columns in six steps of four.  As in
    // k_update_z_mfma16: k = 2 hi + (s2 & 1) within the panel s2 >> 1, so a lane's two entries of a row are one
    // 16-byte load and the four lanes of a row read its 64 bytes; every tile but the first is requested in front
    // of the stores of the tile before it.
    const double* __restrict__ V1p = a_hi > 0 ? V1 : V0;       // (no second panel: its coefficients are zero)
    lazy_coeffs16(beta, ldb, a_lo, a_hi, ucur, uprev, sc);
    double bb[6];
#pragma unroll
    for (int s2 = 0; s2 < 6; ++s2) {
      const int kk = 2 * hi + (s2 & 1);
      const double v = s2 < 2 ? -sc[1280 + kk + 16 * (lo & 7)] : s2 < 4 ? (a_hi > 0 ? -sc[1536 + kk + 16 * (lo & 7)] : 0.0) : sc[1024 + kk + 16 * (lo & 7)];
      bb[s2] = lo < TS ? v : 0.0;
    }
    double2 rg[3];
    size_t t = (size_t)blockIdx.x * (WG / 64) + wave;
    {
      const size_t tl = t < ntile ? t : ntile - 1, arow = (tl << 4) + lo;
      const size_t base = (arow < (size_t)m ? arow : 0) * TS + 2 * hi;
      rg[0] = *reinterpret_cast<const double2*>(V0 + base);
      rg[1] = *reinterpret_cast<const double2*>(V1p + base);
      rg[2] = *reinterpret_cast<const double2*>(Z + base);
    }
    while (t < ntile) {
      const size_t r0 = t << 4;
      const bool aok = r0 + lo < (size_t)m;
      const double a[6] = {aok ? rg[0].x : 0.0, aok ? rg[0].y : 0.0, aok ? rg[1].x : 0.0, aok ? rg[1].y : 0.0,
                           aok ? rg[2].x : 0.0, aok ? rg[2].y : 0.0};
      mfma_d4 z = mfma_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s2 = 0; s2 < 6; ++s2) z = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], bb[s2], z, 0, 0, 0);
      const size_t tn = t + tstride;
      {
        const size_t tl = tn < ntile ? tn : t, arow = (tl << 4) + lo;
        const size_t base = (arow < (size_t)m ? arow : 0) * TS + 2 * hi;
        rg[0] = *reinterpret_cast<const double2*>(V0 + base);
        rg[1] = *reinterpret_cast<const double2*>(V1p + base);
        rg[2] = *reinterpret_cast<const double2*>(Z + base);
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t row = r0 + hi + 4 * r;
        if (row < (size_t)m && lo < nc) Z[row * TS + lo] = z[r];
      }
      t = tn;
    }
    return;
  }
  mfma_d4 zz = mfma_d4{0.0, 0.0, 0.0, 0.0};
  for (size_t t = (size_t)blockIdx.x * (WG / 64) + wave; t < ntile; t += tstride) {
    const size_t r0 = t << 4;
    mfma_d4 z;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t row = r0 + hi + 4 * r;
      z[r] = (row < (size_t)m && lo < TS) ? Z[row * TS + lo] : 0.0;
    }
    const size_t arow = r0 + lo;
    const bool aok = arow < (size_t)m;
    double a[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const int k = 4 * s2 + hi;
      a[s2] = (aok && von[s2]) ? (k < TS ? V0[arow * TS + k] : V1[arow * TS + k - TS]) : 0.0;
    }
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) z = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], bneg[s2], z, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t row = r0 + hi + 4 * r;
      if (row < (size_t)m && lo < nc) Z[row * TS + lo] = z[r];
    }
    if (zzp) update_z_gram_step(z, zz, r0, hi, lo, m, zzc);
  }
  if (zzp) update_z_gram_out<TS>(zz, sc, zzp, wave, lane);
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

// The per-system sums of the stopping test: out[j] = sum over the s columns of system j (ascending) of the sum over
// the blocks of rtr[blk*ts + c] (the column sums of R^2 an update kernel or k_colnorm2 left).  One workgroup; 16
// threads per column take the blocks b = l, l + 16, ... in turn and are folded by a fixed tree, so the k values are
// reproducible.  The values go to device memory and to pinned host words, which the host reads once the launch or
// event behind this one has completed (it keys on nothing this kernel writes).
__global__ __launch_bounds__(WG) void k_group_norms(const double* __restrict__ rtr, int nblk, int ts, int k, int s,
                                                    double* __restrict__ out, double* host) {
  __shared__ double red[WG];
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
  if (threadIdx.x < k) {
    double g = 0.0;
    for (int q = 0; q < s; ++q) g += red[(threadIdx.x * s + q) << 4];
    out[threadIdx.x] = g;
    if (host) __hip_atomic_store(host + threadIdx.x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence_system();
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

inline int grid_rows(int m, int per_thread_rows = 1) {
  long long blocks = ((long long)m + (long long)WG * per_thread_rows - 1) / ((long long)WG * per_thread_rows);
  if (blocks < 1) blocks = 1;
  const long long cap = 2048;
  return (int)(blocks < cap ? blocks : cap);
}

}  // namespace

// Sequence number for the next launch that writes its two words to pinned host memory (host[2] =
// seq behind them): the host then polls that word instead of waiting for an event, whose record
// costs the stream 5-6 us of idle time.  One-shot: taken by that launch, 0 = no number.
static double g_note_seq = 0.0;
static inline double take_note_seq(const double* host) {
  if (!host) return 0.0;
  const double v = g_note_seq;
  g_note_seq = 0.0;
  return v;
}

extern "C" {

/* partial blocks a Gram buffer must hold: the kernels' grid cap + the shares and the ticket of k_finish_wide */
int pa_gram_max_blocks(void) { return GRAM_WIDE_BLOCKS + GRAM_SCRATCH_BLOCKS; }

void pa_k_note_seq(double seq) { g_note_seq = seq; }

int pa_finish32_scratch_blocks(void) { return FIN32_WG + 1; }     /* the shares + the block that holds the ticket */

int pa_k_finish32(const double* partials, int nblk, double* scratch, int t, int T, double* out, double* mu,
                  double* alpha, int* info) {
  PA_LAUNCH(k_finish32, dim3(FIN32_WG), dim3(WG), 0, cur_stream(), partials, nblk, scratch, t, T, out, mu,
            alpha, info, (const double*)nullptr, 0, 0, 0, (double*)nullptr);
  return kfail("k_finish32");
}

int pa_k_finish32_pair(const double* pa, int na, double* sa, int t, int T, double* outa, double* mu, double* alpha,
                       int* info, const double* pb, int nb, double* sb, double* outb) {
  PA_LAUNCH(k_finish32_pair, dim3(2 * FIN32_WG), dim3(WG), 0, cur_stream(), pa, na, sa, t, T, outa, mu, alpha, info,
            pb, nb, sb, outb);
  return kfail("k_finish32_pair");
}

int pa_k_finish32_trace(const double* partials, int nblk, double* scratch, double* out, const double* rtr_partials,
                        int rtr_nblk, int ts, int nc, double* res2, int* info) {
  PA_LAUNCH(k_finish32, dim3(FIN32_WG), dim3(WG), 0, cur_stream(), partials, nblk, scratch, 0, 0, out,
            (double*)nullptr, (double*)nullptr, info, rtr_partials, rtr_nblk, ts, nc, res2);
  return kfail("k_finish32");
}

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

int pa_k_gram(int m, int ts, const double* A0, const double* A1, const double* B, double* partials,
              int* nblk) {
  int blocks = grid_rows(m, 4);
  // (8 columns: up to 1024 workgroups -- four wavefronts per SIMD keep more of the three panel streams in flight:
  // 42.2 -> 38.2 us, the sum of the 1024 partial blocks +1.9 us.  k_gram<4, 2> measured best at 512 in round 2;
  // 16 columns lose with 1024: 69.6 -> 72.5 us and +5 us in the sum.)
  const int cap = ts == 8 ? GRAM_WIDE_BLOCKS : GRAM_MAX_BLOCKS;
  if (blocks > cap) blocks = cap;
  *nblk = blocks;
  if (ts == 16) {   // matrix cores (k_gram_mfma16)
    if (A1) PA_LAUNCH((k_gram_mfma16<2>), dim3(blocks), dim3(WG), 0, cur_stream(), m, A0, A1, B, partials);
    else PA_LAUNCH((k_gram_mfma16<1>), dim3(blocks), dim3(WG), 0, cur_stream(), m, A0, A1, B, partials);
    return kfail("k_gram_mfma16");
  }
  if (ts == 8) {
    if (A1) PA_LAUNCH((k_gram_mfma8<2>), dim3(blocks), dim3(WG), 0, cur_stream(), m, A0, A1, B, partials);
    else PA_LAUNCH((k_gram_mfma8<1>), dim3(blocks), dim3(WG), 0, cur_stream(), m, A0, A1, B, partials);
    return kfail("k_gram_mfma8");
  }
  if (A1) {
    TS_DISPATCH(ts, PA_LAUNCH((k_gram<TS_, 2>), dim3(blocks), dim3(WG), 0, cur_stream(), m,
                                       A0, A1, B, partials));
  } else {
    TS_DISPATCH(ts, PA_LAUNCH((k_gram<TS_, 1>), dim3(blocks), dim3(WG), 0, cur_stream(), m,
                                       A0, A1, B, partials));
  }
  return kfail("k_gram");
}

/* The sum of wide partial blocks by FINW_WG workgroups (k_finish_wide); the shares and the ticket lie behind the
 * GRAM_WIDE_BLOCKS partial blocks of the buffer (pa_gram_max_blocks() counts them in). */
static int finish_wide(const double* partials, int nblk, int npan, int ts, int a_lo, int a_hi, int nb, double* out,
                       int ld_out, int t, int T, double* mu, double* alpha, int* info, const double* rtr, int rtr_nblk,
                       int rtr_nc, double* res2) {
  double* scratch = const_cast<double*>(partials) + (size_t)GRAM_WIDE_BLOCKS * 2 * ts * ts;
  PA_LAUNCH(k_finish_wide, dim3(FINW_WG), dim3(WG), 0, cur_stream(), partials, nblk, npan, ts, a_lo, a_hi, nb, out, ld_out,
            scratch, t, T, mu, alpha, info, rtr, rtr_nblk, rtr_nc, res2);
  return kfail("k_finish_wide");
}

int pa_k_gram_finish(int m, int ts, const double* A0, const double* A1, const double* B,
                     double* partials, int a_lo, int a_hi, int nb, double* out, int ld_out, int t,
                     int T, double* mu, double* alpha, int* info) {
  int nblk = 0;
  if ((a_lo + a_hi) * nb <= 0) return 0;
  if (pa_k_gram(m, ts, A0, A1, B, partials, &nblk)) return 1;
  if (ts >= 8) {
    if (t > 0 && (a_lo != t || a_hi != T || nb != t || ld_out != t + T || !A1)) {
      snprintf(g_kerr, sizeof(g_kerr), "pa_k_gram_finish: [W ; G^T] layout expected");
      return 1;
    }
    return finish_wide(partials, nblk, A1 ? 2 : 1, ts, a_lo, a_hi, nb, out, ld_out, t, T, mu, alpha, info, nullptr, 0, 0, nullptr);
  }
  if (t > 0) {
    if (a_lo != t || a_hi != T || nb != t || ld_out != t + T || !A1) {
      snprintf(g_kerr, sizeof(g_kerr), "pa_k_gram_finish: [W ; G^T] layout expected");
      return 1;
    }
    if ((t + T) * t > 128) {   // large block: spread the sum, then factor
      if (pa_k_finish(partials, nblk, 2, ts, t, T, t, out, t + T)) return 1;
      return pa_k_potrf_alpha(out, t, T, mu, alpha, info);
    }
    PA_LAUNCH(k_finish_potrf_alpha, dim3(1), dim3(1024), 0, cur_stream(), partials, nblk, 2, ts,
                       t, T, out, mu, alpha, info);
    return kfail("k_finish_potrf_alpha");
  }
  return pa_k_finish(partials, nblk, A1 ? 2 : 1, ts, a_lo, a_hi, nb, out, ld_out);
}

int pa_k_gram_finish_trace(int m, int ts, const double* A0, const double* A1, const double* B, double* partials,
                           int a_lo, int a_hi, int nb, double* out, int ld_out, const double* rtr_partials,
                           int rtr_nblk, int nc, double* res2, const int* info) {
  int nblk = 0;
  const int ne = (a_lo + a_hi) * nb;
  if (ne > 0 && ts >= 8) {     /* wide blocks: several workgroups sum, the last one adds the norm */
    if (pa_k_gram(m, ts, A0, A1, B, partials, &nblk)) return 1;
    return finish_wide(partials, nblk, A1 ? 2 : 1, ts, a_lo, a_hi, nb, out, ld_out, 0, 0, nullptr, nullptr, const_cast<int*>(info),
                       rtr_partials, rtr_nblk, nc, res2);
  }
  if (ne <= 0 || ne > 128)     /* no Gram block, or one that several workgroups sum: the two launches */
    return pa_k_trace_finish(rtr_partials, rtr_nblk, ts, nc, res2, info, NULL) ||
           pa_k_gram_finish(m, ts, A0, A1, B, partials, a_lo, a_hi, nb, out, ld_out, 0, 0, NULL, NULL, NULL);
  if (pa_k_gram(m, ts, A0, A1, B, partials, &nblk)) return 1;
  PA_LAUNCH(k_finish_trace, dim3(1), dim3(1024), 0, cur_stream(), partials, nblk, A1 ? 2 : 1, ts, a_lo, a_hi, nb,
            out, ld_out, rtr_partials, rtr_nblk, nc, res2, info);
  return kfail("k_finish_trace");
}

int pa_k_finish(const double* partials, int nblk, int npan, int ts, int a_lo, int a_hi, int nb,
                double* out, int ld_out) {
  const int ne = (a_lo + a_hi) * nb;
  if (ne <= 0) return 0;
  // wide blocks in the Gram buffer of a solver (pa_gram_max_blocks() blocks: the shares and the ticket of
  // k_finish_wide lie behind them) -- BF-Omin's Z^T Z, up to 2048 blocks from the update kernel
  if (ts >= 8 && (long long)nblk * npan * ts * ts <= (long long)GRAM_WIDE_BLOCKS * 2 * ts * ts)
    return finish_wide(partials, nblk, npan, ts, a_lo, a_hi, nb, out, ld_out, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr);
  const int groups = ne > 128 ? (ne + 63) / 64 : 1;    // one workgroup unless the block is large
  PA_LAUNCH(k_finish, dim3(groups), dim3(1024), 0, cur_stream(), partials, nblk, npan, ts, a_lo,
                     a_hi, nb, out, ld_out);
  return kfail("k_finish");
}

int pa_k_potrf(double* W, int t, int* info) {
  PA_LAUNCH(k_potrf, dim3(1), dim3(64), 0, cur_stream(), W, t, info);
  return kfail("k_potrf");
}

int pa_k_fused_small(double* mu, int t, int nrhs, int bm, int bn, int ldb, double* alpha,
                     double* beta, int* info) {
  PA_LAUNCH(k_fused_small, dim3(1), dim3(64), 0, cur_stream(), mu, t, nrhs, bm, bn, ldb,
                     alpha, beta, info);
  return kfail("k_fused_small");
}

int pa_k_trsm(int m, int ts, int t, const double* U, double* P, double* AP) {
  if (t <= 0) return 0;
  TS_DISPATCH(ts, PA_LAUNCH((k_trsm<TS_>), dim3(grid_rows(m)), dim3(WG), 0, cur_stream(),
                                     m, t, U, P, AP));
  return kfail("k_trsm");
}

int pa_k_update_xr(int m, int ts, int t, int nc, const double* alpha, const double* P,
                   const double* AP, double* X, double* R, double* rtr_partials, int* nblk,
                   int trace_nc, double* res2, const int* info, double* host) {
  int blocks = grid_rows(m, 2);
  if (blocks > GRAM_MAX_BLOCKS) blocks = GRAM_MAX_BLOCKS;
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_update_xr<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m,
                                     t, nc, alpha, P, AP, X, R, rtr_partials));
  if (kfail("k_update_xr")) return 1;
  if (trace_nc <= 0) return 0;
  PA_LAUNCH(k_trace_finish, dim3(1), dim3(WG), 0, cur_stream(), rtr_partials, blocks, ts, trace_nc,
                     res2, info, host, take_note_seq(host));
  return kfail("k_trace_finish");
}

int pa_k_potrf_alpha(const double* buf, int t, int T, double* mu, double* alpha, int* info) {
  PA_LAUNCH(k_potrf_alpha, dim3(1), dim3(64), 0, cur_stream(), buf, t, T, mu, alpha, info);
  return kfail("k_potrf_alpha");
}

/* The grid of k_trsm_update and k_update_xrz: the layout of their column sums of R^2 (and so the norm summed from
 * them) depends on it. */
static int update_grid(int m) {
  int blocks = grid_rows(m, 2);
  return blocks > GRAM_MAX_BLOCKS ? GRAM_MAX_BLOCKS : blocks;
}
/* X with the nontemporal hint (k_trsm_update): only a panel of 16 MiB or more; a smaller one stays in the caches */
static int x_nontemporal(int m, int ts) { return (size_t)m * ts * sizeof(double) >= ((size_t)16 << 20) ? 1 : 0; }

int pa_k_trsm_update(int m, int ts, int t, int nc, double* U, double* alpha, double* P,
                     double* AP, double* X, double* R, double* rtr_partials, int* nblk, int trace_nc,
                     double* res2, int* info, double* host, const double* gram, double* ukeep) {
  const int blocks = update_grid(m);
  *nblk = blocks;
  // PREALPS_TRSM_MFMA=0: lane-per-row substitution at every width (the matrix-core variant forms U^-1)
  static int use_mfma = -1;
  if (use_mfma < 0) { const char* e = getenv("PREALPS_TRSM_MFMA"); use_mfma = e ? atoi(e) : 1; }
  if (ts == 16 && use_mfma)
    PA_LAUNCH((k_trsm_update_mfma<16>), dim3(blocks), dim3(WG), 0, cur_stream(), m, t, nc, U, alpha, P, AP, X, R, rtr_partials, gram, info, ukeep);
  else if (ts == 8 && use_mfma)
    PA_LAUNCH((k_trsm_update_mfma<8>), dim3(blocks), dim3(WG), 0, cur_stream(), m, t, nc, U, alpha, P, AP, X, R, rtr_partials, gram, info, ukeep);
  else {
    TS_DISPATCH(ts, PA_LAUNCH((k_trsm_update<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m,
                                       t, nc, U, alpha, P, AP, X, R, rtr_partials, gram, info, ukeep,
                                       x_nontemporal(m, ts)));
  }
  if (kfail("k_trsm_update")) return 1;
  if (trace_nc <= 0) return 0;
  PA_LAUNCH(k_trace_finish, dim3(1), dim3(WG), 0, cur_stream(), rtr_partials, blocks, ts, trace_nc,
                     res2, (const int*)info, host, take_note_seq(host));
  return kfail("k_trace_finish");
}

int pa_k_update_xrz(int m, int ts, int t, double* U, double* alpha, const double* P, const double* AP,
                    const double* P_prev, double* X, double* R, double* Z, double* rtr_partials, int* nblk,
                    double* ukeep, const double* beta, int ldb, const double* uprev) {
  if (ts != 4 || t < 1 || t > 4 || ldb < 2 * t || !U || !alpha || !P_prev || !ukeep || !beta || !uprev) {
    snprintf(g_kerr, sizeof(g_kerr), "pa_k_update_xrz: 4-column panels with lazy normalisation only");
    return 1;
  }
  const int blocks = update_grid(m);
  *nblk = blocks;
  PA_LAUNCH((k_update_xrz<4>), dim3(blocks), dim3(WG), 0, cur_stream(), m, t, U, alpha, P, AP, P_prev, X, R, Z,
            rtr_partials, ukeep, beta, ldb, uprev, x_nontemporal(m, ts));
  return kfail("k_update_xrz");
}

int pa_k_colnorm2(int m, int ts, const double* R, double* rtr_partials, int* nblk) {
  int blocks = grid_rows(m, 4);
  if (blocks > GRAM_MAX_BLOCKS) blocks = GRAM_MAX_BLOCKS;
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_colnorm2<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m,
                                     R, rtr_partials));
  return kfail("k_colnorm2");
}

int pa_k_trace_finish(const double* rtr_partials, int nblk, int ts, int nc, double* res2,
                      const int* info, double* host) {
  PA_LAUNCH(k_trace_finish, dim3(1), dim3(WG), 0, cur_stream(), rtr_partials, nblk, ts, nc,
                     res2, info, host, take_note_seq(host));
  return kfail("k_trace_finish");
}

/* One-shot: the next pa_k_update_z on a panel of up to 4 columns also packs the send rows of the Z it writes
 * (pa_operator_pack_hint).  Returns 0 when that launch would not take it (wider panels). */
static struct { const int* off; const int* slot; double* buf; } g_zpack;
int pa_k_update_z_pack(int ts, const int* pk_off, const int* pk_slot, double* sendbuf) {
  g_zpack.off = g_zpack.slot = nullptr; g_zpack.buf = nullptr;
  if (ts > 4 || !pk_off || !pk_slot || !sendbuf) return 0;
  g_zpack.off = pk_off; g_zpack.slot = pk_slot; g_zpack.buf = sendbuf;
  return 1;
}

int pa_k_update_z(int m, int ts, int a_lo, int a_hi, int nc, const double* beta, int ldb,
                  const double* V0, const double* V1, double* Z, const double* note_src, double* note_host,
                  const double* ucur, const double* uprev, double* zz_part, int zz_cols, int* zz_nblk) {
  const auto pk = g_zpack;
  g_zpack.off = g_zpack.slot = nullptr; g_zpack.buf = nullptr;
  if (zz_nblk) *zz_nblk = 0;
  if (nc <= 0) return 0;
  if (ucur && (!uprev || nc != a_lo || (a_hi != 0 && a_hi != a_lo))) {
    snprintf(g_kerr, sizeof(g_kerr), "pa_k_update_z: lazy normalisation needs square blocks");
    return 1;
  }
  const double seq_ = take_note_seq(note_host);
  // zz_part (8 / 16 columns, panels normalised in place): the launch also leaves Z^T Z of the new Z behind, one
  // ts x ts block per workgroup (*zz_nblk of them, the partial blocks pa_k_finish sums); elsewhere *zz_nblk stays 0
  double* zzp = (zz_part && zz_nblk && !ucur && (ts == 8 || ts == 16)) ? zz_part : nullptr;
  if (ts == 16) {   // matrix cores (k_update_z_mfma16), one 16-row tile per wavefront and step
    const int grid = grid_rows(m, 4);
    PA_LAUNCH(k_update_z_mfma16, dim3(grid), dim3(WG), 0, cur_stream(), m, a_lo, a_hi, nc,
                       beta, ldb, V0, V1, Z, note_src, note_host, seq_, ucur, uprev, zzp, zz_cols);
    if (zzp) *zz_nblk = grid;
    return kfail("k_update_z_mfma16");
  }
  if (ts == 8) {
    const int grid = grid_rows(m, 4);
    PA_LAUNCH(k_update_z_mfma8, dim3(grid), dim3(WG), 0, cur_stream(), m, a_lo, a_hi, nc,
                       beta, ldb, V0, V1, Z, note_src, note_host, seq_, ucur, uprev, zzp, zz_cols);
    if (zzp) *zz_nblk = grid;
    return kfail("k_update_z_mfma8");
  }
  TS_DISPATCH(ts, PA_LAUNCH((k_update_z<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0,
                                     cur_stream(), m, a_lo, a_hi, nc, beta, ldb, V0, V1, Z, note_src, note_host, seq_, ucur, uprev,
                                     pk.off, pk.slot, pk.buf));
  return kfail("k_update_z");
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
  snprintf(g_kerr, sizeof(g_kerr), "%s: %d systems of %d columns do not fit a panel of stride %d", what, k, s, ts);
  return 1;
}

int pa_k_multi_start(int m, int ts, int k, int s, const double* B, int ldb, const int* pcol, double* R,
                     double* sums, int* nblk) {
  if (multi_args_bad("pa_k_multi_start", ts, k, s)) return 1;
  int blocks = grid_rows(m, 4);
  if (blocks > GRAM_MAX_BLOCKS) blocks = GRAM_MAX_BLOCKS;
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
  int blocks = grid_rows(m, 4);      // (the grid of pa_k_multi_start: the same partial sums of B^2)
  if (blocks > GRAM_MAX_BLOCKS) blocks = GRAM_MAX_BLOCKS;
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

int pa_k_rowsum_groups(int m, int ts, int k, int s, const double* X, double* sol, int ld) {
  if (multi_args_bad("pa_k_rowsum_groups", ts, k, s)) return 1;
  TS_DISPATCH(ts, PA_LAUNCH((k_rowsum_groups<TS_>), dim3(grid_rows(m, 2)), dim3(WG), 0, cur_stream(), m, k, s, X,
                            sol, (size_t)ld));
  return kfail("k_rowsum_groups");
}

}  // extern "C"
