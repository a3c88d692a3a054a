// dense_update.hip -- the dense updates of the ECG block iteration, with their C launchers (pa_device.h):
//  - X / R: the triangular solve of P / AP, X += P alpha, R -= AP alpha with the column sums of R^2, in separate
//    kernels and in one pass (k_trsm_update; on the matrix cores at 8 / 16 columns);
//  - Z -= [V0 | V1] beta: lane per row up to 4 columns, on the matrix cores at 8 / 16, with the lazy normalisation,
//    the packing of the send rows (g_zpack) and Z^T Z as by-products;
//  - k_update_xrz, which is both in one pass and so keeps the two halves in one unit; it moves X in every pass or in
//    every second one (its X modes), and k_flush_x pays an update of X that a stop left owed.
// See dense_gram.hip for the layout of panels and blocks.
#include "dense_device.h"

namespace {
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
  // (note_host: the all-reduced residual norm and the factorisation status next to beta)
  if (note_host && blockIdx.x == 0 && threadIdx.x == 0) note_to_host(note_host, note_src, note_seq);
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
//
// XM, what the pass does with X (ecg_loops.c: solve_first_step decides, pa_ecg_x_mode).  Nobody reads X between two row
// passes of one call of the library's loops, so its 2 x 33 MB need not move in every pass:
//   XM_EVERY  x += p alpha, as k_trsm_update;
//   XM_SKIP   X is neither read nor written: the update is owed.  U is in ukeep and P stays raw, as ever; workgroup 0
//             keeps alpha in akeep, because the finish of the next iteration overwrites it;
//   XM_BOTH   the owed update first -- the raw P_prev row normalised with U_prev (sfac's second half, already here for
//             Z) by trsm_update_row's own loop, x += p_prev alpha_prev with alpha_prev from akeep -- then this
//             iteration's: the two additions to x[c] of two XM_EVERY passes, in their order, so the same bits.
// k_flush_x pays a debt no pass will pay (a stop).  xnt holds wherever X moves.
enum { XM_EVERY = 0, XM_SKIP = 1, XM_BOTH = 2 };
// The owed update of one row: p (raw, of the factor su; sd = 1 / its diagonal) <- p U^-1, x += p alpha.  This IS
// trsm_update_row -- on an AP, an R and column sums that nobody reads, which the compiler drops.
template <int TS>
__device__ __forceinline__ void owed_x_row(double (&p)[TS], double (&x)[TS], const double* su, const double* sd,
                                           const double* sa, int t) {
  double ap[TS], r[TS], rr[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) ap[c] = r[c] = rr[c] = 0.0;
  trsm_update_row<TS>(p, ap, x, r, rr, su, sd, sa, t, t);
}
template <int TS, int XM>
__global__ __launch_bounds__(WG) void k_update_xrz(int m, int t, double* U, double* alpha, const double* __restrict__ P,
                                                   const double* __restrict__ AP, const double* __restrict__ Pprev,
                                                   double* __restrict__ X, double* __restrict__ R,
                                                   double* __restrict__ Z, double* __restrict__ rtr,
                                                   double* __restrict__ ukeep, const double* __restrict__ beta,
                                                   int ldb, const double* __restrict__ uprev, int xnt,
                                                   double* __restrict__ akeep) {
  __shared__ double su[TS * TS];
  __shared__ double sd[TS];
  __shared__ double sa[TS * TS];
  __shared__ double sb[2 * TS * TS];
  __shared__ double sfac[2 * TS * TS];
  __shared__ double sc[7 * TS * TS];
  __shared__ double sdp[TS];          // XM_BOTH: 1 / diag(U_prev) and alpha_prev
  __shared__ double sap[TS * TS];
  const int na = 2 * t, tt = t * t;
  for (int e = threadIdx.x; e < na * t; e += WG) sb[e] = beta[(e % na) + ldb * (e / na)];
  for (int e = threadIdx.x; e < 2 * tt; e += WG) sfac[e] = e < tt ? U[e] : uprev[e - tt];
  if (XM == XM_BOTH) for (int e = threadIdx.x; e < tt; e += WG) sap[e] = akeep[e];
  trsm_update_prologue<TS>(t, t, U, alpha, nullptr, nullptr, ukeep, su, sd, sa);    // (its barriers cover sb / sfac / sap)
  if (XM == XM_SKIP && blockIdx.x == 0) for (int e = threadIdx.x; e < tt; e += WG) akeep[e] = sa[e];
  if (XM == XM_BOTH && threadIdx.x < t) sdp[threadIdx.x] = 1.0 / sfac[tt + threadIdx.x + t * threadIdx.x];   // (sd's own expression)
  lazy_coeffs_wg<TS>(sb, sfac, t, t, sc);      // (ends with a barrier: sdp is there)
  const double* C0 = sc + 4 * TS * TS; const double* C1 = sc + 5 * TS * TS; const double* C2 = sc + 6 * TS * TS;
  double rr[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) rr[c] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double p[TS], ap[TS], x[TS], r[TS], z[TS], v0[TS], v1[TS], o[TS];
    load_row<TS>(P, row, v0);
    load_row<TS>(AP, row, ap);
    if (XM == XM_SKIP) {
#pragma unroll
      for (int c = 0; c < TS; ++c) x[c] = 0.0;      // (never stored: the X half of the row code falls away)
    } else if (xnt) load_row_nt<TS>(X, row, x); else load_row<TS>(X, row, x);
    load_row<TS>(R, row, r);
    load_row<TS>(Z, row, z);
    load_row<TS>(Pprev, row, v1);
    if (XM == XM_BOTH) {
#pragma unroll
      for (int c = 0; c < TS; ++c) p[c] = v1[c];
      owed_x_row<TS>(p, x, sfac + tt, sdp, sap, t);
    }
#pragma unroll
    for (int c = 0; c < TS; ++c) p[c] = v0[c];      // (normalised in registers below; Z's update takes the raw row)
    trsm_update_row<TS>(p, ap, x, r, rr, su, sd, sa, t, t);
    update_z_lazy_row<TS>(z, v0, v1, o, C0, C1, C2, t, t, t);
    if (XM != XM_SKIP) { if (xnt) store_row_nt<TS>(X, row, x); else store_row<TS>(X, row, x); }
    store_row<TS>(R, row, r);
    store_row<TS>(Z, row, o);
  }
  block_sum_cols<TS>(rr, rtr + (size_t)blockIdx.x * TS);
}

// X += (P_prev U_prev^-1) alpha_prev: the update a k_update_xrz<XM_SKIP> pass owes, where no XM_BOTH pass follows it.
template <int TS>
__global__ __launch_bounds__(WG) void k_flush_x(int m, int t, const double* __restrict__ uprev,
                                                const double* __restrict__ akeep, const double* __restrict__ Pprev,
                                                double* __restrict__ X, int xnt) {
  __shared__ double su[TS * TS];
  __shared__ double sd[TS];
  __shared__ double sa[TS * TS];
  for (int e = threadIdx.x; e < t * t; e += WG) { su[e] = uprev[e]; sa[e] = akeep[e]; }
  __syncthreads();
  if (threadIdx.x < t) sd[threadIdx.x] = 1.0 / su[threadIdx.x + t * threadIdx.x];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double p[TS], x[TS];
    load_row<TS>(Pprev, row, p);
    if (xnt) load_row_nt<TS>(X, row, x); else load_row<TS>(X, row, x);
    owed_x_row<TS>(p, x, su, sd, sa, t);
    if (xnt) store_row_nt<TS>(X, row, x); else store_row<TS>(X, row, x);
  }
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
  // (note_host: the all-reduced residual norm and the factorisation status next to beta)
  if (note_host && blockIdx.x == 0 && threadIdx.x == 0) note_to_host(note_host, note_src, note_seq);
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
  // (note_host: the all-reduced residual norm and the factorisation status next to beta)
  if (note_host && blockIdx.x == 0 && threadIdx.x == 0) note_to_host(note_host, note_src, note_seq);
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

}  // namespace

extern "C" {

int pa_k_trsm(int m, int ts, int t, const double* U, double* P, double* AP) {
  if (t <= 0) return 0;
  TS_DISPATCH(ts, PA_LAUNCH((k_trsm<TS_>), dim3(grid_rows(m)), dim3(WG), 0, cur_stream(),
                                     m, t, U, P, AP));
  return kfail("k_trsm");
}

int pa_k_update_xr(int m, int ts, int t, int nc, const double* alpha, const double* P,
                   const double* AP, double* X, double* R, double* rtr_partials, int* nblk,
                   int trace_nc, double* res2, const int* info, double* host) {
  const int blocks = update_grid(m);
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_update_xr<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m,
                                     t, nc, alpha, P, AP, X, R, rtr_partials));
  if (kfail("k_update_xr")) return 1;
  if (trace_nc <= 0) return 0;
  return pa_k_trace_finish(rtr_partials, blocks, ts, trace_nc, res2, info, host);
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
  return pa_k_trace_finish(rtr_partials, blocks, ts, trace_nc, res2, info, host);
}

int pa_k_update_xrz_mode(int m, int ts, int t, double* U, double* alpha, const double* P, const double* AP,
                         const double* P_prev, double* X, double* R, double* Z, double* rtr_partials, int* nblk,
                         double* ukeep, const double* beta, int ldb, const double* uprev, int xmode, double* akeep) {
  if (ts != 4 || t < 1 || t > 4 || ldb < 2 * t || !U || !alpha || !P_prev || !ukeep || !beta || !uprev) {
    pa_rt_set_error("pa_k_update_xrz: 4-column panels with lazy normalisation only");
    return 1;
  }
  if (xmode < XM_EVERY || xmode > XM_BOTH || (xmode != XM_EVERY && !akeep)) {
    pa_rt_set_error("pa_k_update_xrz: X mode %d, or no place for the kept alpha", xmode);
    return 1;
  }
  const int blocks = update_grid(m);
  *nblk = blocks;
  const int xnt = x_nontemporal(m, ts);
  if (xmode == XM_SKIP)
    PA_LAUNCH((k_update_xrz<4, XM_SKIP>), dim3(blocks), dim3(WG), 0, cur_stream(), m, t, U, alpha, P, AP, P_prev, X, R, Z,
              rtr_partials, ukeep, beta, ldb, uprev, xnt, akeep);
  else if (xmode == XM_BOTH)
    PA_LAUNCH((k_update_xrz<4, XM_BOTH>), dim3(blocks), dim3(WG), 0, cur_stream(), m, t, U, alpha, P, AP, P_prev, X, R, Z,
              rtr_partials, ukeep, beta, ldb, uprev, xnt, akeep);
  else
    PA_LAUNCH((k_update_xrz<4, XM_EVERY>), dim3(blocks), dim3(WG), 0, cur_stream(), m, t, U, alpha, P, AP, P_prev, X, R, Z,
              rtr_partials, ukeep, beta, ldb, uprev, xnt, akeep);
  return kfail("k_update_xrz");
}
int pa_k_update_xrz(int m, int ts, int t, double* U, double* alpha, const double* P, const double* AP,
                    const double* P_prev, double* X, double* R, double* Z, double* rtr_partials, int* nblk,
                    double* ukeep, const double* beta, int ldb, const double* uprev) {
  return pa_k_update_xrz_mode(m, ts, t, U, alpha, P, AP, P_prev, X, R, Z, rtr_partials, nblk, ukeep, beta, ldb, uprev,
                              XM_EVERY, nullptr);
}

int pa_k_flush_x(int m, int ts, int t, const double* uprev, const double* akeep, const double* P_prev, double* X) {
  if (ts != 4 || t < 1 || t > 4 || !uprev || !akeep || !P_prev || !X) {
    pa_rt_set_error("pa_k_flush_x: 4-column panels with a kept factor and a kept alpha only");
    return 1;
  }
  PA_LAUNCH((k_flush_x<4>), dim3(update_grid(m)), dim3(WG), 0, cur_stream(), m, t, uprev, akeep, P_prev, X,
            x_nontemporal(m, ts));
  return kfail("k_flush_x");
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
    pa_rt_set_error("pa_k_update_z: lazy normalisation needs square blocks");
    return 1;
  }
  const double seq_ = pa_k_take_note_seq(note_host);
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

}  // extern "C"
