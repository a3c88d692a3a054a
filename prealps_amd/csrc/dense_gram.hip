// dense_gram.hip -- the Gram products of the ECG block iteration and what finishes them: the sum of the
// per-workgroup partial blocks, the Cholesky factor and alpha, the column norms and the residual norm, with their
// C launchers (pa_device.h) and the one-shot sequence number of the note to a polling host (g_note_seq).
// All panels are row-interleaved [rows][TS] fp64, all small t x t blocks column-major like the reference's work
// area.  Every kernel of the dense units is HBM-bandwidth bound (the tall-skinny kernels t/8..t/4 flop/B against a
// ridge of ~10 flop/B): coalesced 16-B accesses, LDS staging where rows are reused, 64-wide shuffle reductions.
// The X / R / Z updates are dense_update.hip, the column utilities, the starts of several systems and the HBM
// probes dense_panels.hip; what they share is dense_device.h.
#include "dense_device.h"

namespace {
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
    const double words[2] = {r2, st};
    if (host) note_to_host(host, words, seq);
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

__global__ void k_potrf_alpha(const double* __restrict__ buf, int t, int T, double* __restrict__ mu,
                              double* __restrict__ alpha, int* __restrict__ info) {
  __shared__ double W[16 * 16];
  __shared__ double G[16 * 16];
  potrf_alpha_wg(buf, t, T, mu, alpha, info, W, G);
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

}  // namespace

extern "C" {

/* partial blocks a Gram buffer must hold: the kernels' grid cap + the shares and the ticket of k_finish_wide */
int pa_gram_max_blocks(void) { return GRAM_WIDE_BLOCKS + GRAM_SCRATCH_BLOCKS; }

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

int pa_k_gram(int m, int ts, const double* A0, const double* A1, const double* B, double* partials,
              int* nblk) {
  // (8 columns: up to 1024 workgroups -- four wavefronts per SIMD keep more of the three panel streams in flight:
  // 42.2 -> 38.2 us, the sum of the 1024 partial blocks +1.9 us.  k_gram<4, 2> measured best at 512 in round 2;
  // 16 columns lose with 1024: 69.6 -> 72.5 us and +5 us in the sum.)
  const int blocks = update_grid(m, 4, ts == 8 ? GRAM_WIDE_BLOCKS : GRAM_MAX_BLOCKS);
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
  if (t > 0 && (a_lo != t || a_hi != T || nb != t || ld_out != t + T || !A1)) {
    pa_rt_set_error("pa_k_gram_finish: [W ; G^T] layout expected");
    return 1;
  }
  if (ts >= 8)
    return finish_wide(partials, nblk, A1 ? 2 : 1, ts, a_lo, a_hi, nb, out, ld_out, t, T, mu, alpha, info, nullptr, 0, 0, nullptr);
  if (t > 0) {
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

int pa_k_potrf_alpha(const double* buf, int t, int T, double* mu, double* alpha, int* info) {
  PA_LAUNCH(k_potrf_alpha, dim3(1), dim3(64), 0, cur_stream(), buf, t, T, mu, alpha, info);
  return kfail("k_potrf_alpha");
}

int pa_k_colnorm2(int m, int ts, const double* R, double* rtr_partials, int* nblk) {
  const int blocks = update_grid(m, 4);
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_colnorm2<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m,
                                     R, rtr_partials));
  return kfail("k_colnorm2");
}

// Sequence number for the next launch that writes its two words to pinned host memory (host[2] =
// seq behind them): the host then polls that word instead of waiting for an event, whose record
// costs the stream 5-6 us of idle time.  One-shot: taken by that launch, 0 = no number.
static double g_note_seq = 0.0;
void pa_k_note_seq(double seq) { g_note_seq = seq; }
double pa_k_take_note_seq(const double* host) {
  if (!host) return 0.0;
  const double v = g_note_seq;
  g_note_seq = 0.0;
  return v;
}

int pa_k_trace_finish(const double* rtr_partials, int nblk, int ts, int nc, double* res2,
                      const int* info, double* host) {
  PA_LAUNCH(k_trace_finish, dim3(1), dim3(WG), 0, cur_stream(), rtr_partials, nblk, ts, nc,
                     res2, info, host, pa_k_take_note_seq(host));
  return kfail("k_trace_finish");
}

}  // extern "C"
