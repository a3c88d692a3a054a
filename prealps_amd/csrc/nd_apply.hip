// nd_apply.hip -- CDNA4 (gfx950) sparse block solve for large diagonal blocks: the level-by-level
// sweeps over the nested-dissection factor of nd.c, and the kernel that rounds that factor to fp32.
//
// Sparse block solve with the nested-dissection factor of nd.c.  Every front (n pivot columns,
// m rows below) is stored as the panel P = [T ; -G], T = strictly lower part of (L_11 D^-1)^-1,
// G = (L_21 D^-1) (L_11 D^-1)^-1, D = diag(L_11) -- the "selective inversion" form of a supernodal
// factor: both sweeps become products of dense panels with short vectors, there is no recurrence
// inside a front and one launch takes a whole level of the tree.
//   forward   w = x(pivot rows) + children's contributions;  a = w + T w;  y = D^-1 a  -> Y
//             contribution to the parent = children's contributions(rows below) + (-G) w
//   backward  v = [D^-1 y ; z(rows below, final)];  z_k = v_k + sum_{i > k} P(i, k) v_i
// Two copies of P: column major (forward: a thread owns a front row, lanes = consecutive rows) and
// row major (backward: a thread owns a pivot column, lanes = consecutive columns).
//
// Storage type T of the two copies: double (default) or float (PREALPS_BJ_ND_PRECISION=single, nd.c).
// A float coefficient is widened to double where it is used (v_cvt_f64_f32, exact); every product,
// sum, the LDS staging of w / v and every store stay fp64.  The float copies are rounded from the same
// fp64 values (k_nd_round), so the backward copy is still the exact transpose of the forward one and the
// preconditioner stays symmetric positive definite.
#include "kernels_common.h"

namespace {

// A thread adds coefficient(j) * ys[j] over G-wide groups of an index range (j = G g + u, kept
// to lo <= j < hi); consecutive j are `stride` entries apart at p.  Q threads (wavefronts) share
// one output, groups dealt round robin, and meet in LDS afterwards.  The vector is staged in LDS
// in rounds; the coefficients of a group are requested one group ahead, across the rounds'
// barriers: 128 bytes per thread and group, 16 doubles or 32 floats (G = 32 requests the bytes of
// the fp64 kernels with about their registers).  Each load sits behind its condition and the
// multiplications start behind a full wait, so the requests of the next group do not overlap the
// current group's multiplications; unconditional fp32 loads from a clamped index measured slower
// (DESIGN.md section 4c).
template <typename T> constexpr int nd_group_log2() { return sizeof(T) == 8 ? 4 : 5; }

template <typename T, int G>
__device__ __forceinline__ void nd_dot_load(T (&cf)[G], const T* __restrict__ p, size_t stride, int g, int gtot,
                                            int lo, int hi, bool on) {
#pragma unroll
  for (int u = 0; u < G; ++u) {
    const int j = G * g + u;
    cf[u] = (on && g < gtot && j >= lo && j < hi) ? p[(size_t)j * stride] : T(0);
  }
}

template <int TS, int Q, int YN, typename T, int G>
__device__ __forceinline__ void nd_dot(double (&acc)[TS], T (&cf)[G], const T* __restrict__ p, size_t stride,
                                       int& g, int gend, int gtot, int lo, int hi, bool on, const double (*ys)[TS],
                                       int y0) {
  T nx[G];
#pragma unroll 1
  for (; g < gend; g += Q) {
    nd_dot_load<T, G>(nx, p, stride, g + Q, gtot, lo, hi, on);
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const double cu = (double)cf[u];
      const double2* yq = reinterpret_cast<const double2*>(ys[min(G * g + u - y0, YN - 1)]);
#pragma unroll
      for (int c = 0; c < TS / 2; ++c) {
        const double2 yv = yq[c];
        acc[2 * c] = fma(cu, yv.x, acc[2 * c]);
        acc[2 * c + 1] = fma(cu, yv.y, acc[2 * c + 1]);
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) cf[u] = nx[u];
  }
}

template <typename T>
struct nd_args {
  const int* n; const int* m; const int* ld; const long long* offF; const long long* offB; const int* rows_off;
  const int* coff; const int* ccoff; const int* rows; const int* src; const double* dinv; const T* F;
  const T* B; double* contrib; double* Y;
};
constexpr int ND_CHUNK = 256;                 /* front rows per forward workgroup */
constexpr int ND_COLS = 64;                   /* pivot columns per backward workgroup */
constexpr int ND_STAGE = 512;                 /* entries of w staged per round (forward) */

template <int TS, int XS, typename T>
__device__ __forceinline__ void nd_gather_w(const nd_args<T>& a, const int* __restrict__ rows, const int* __restrict__ src,
                                            int cc0, int cc1, int j, int n, const double* __restrict__ in, int coff,
                                            double (&w)[TS]) {
  const int s0 = src[2 * j], s1 = src[2 * j + 1];
  if (j < n) load_row_s<TS, XS>(in + coff, (size_t)rows[j], w);
  double t[TS];
  if (s0 >= 0) {
    load_row_s<TS, XS>(a.contrib + coff, (size_t)(cc0 + s0), t);
#pragma unroll
    for (int c = 0; c < TS; ++c) w[c] += t[c];
  }
  if (s1 >= 0) {
    load_row_s<TS, XS>(a.contrib + coff, (size_t)(cc1 + s1), t);
#pragma unroll
    for (int c = 0; c < TS; ++c) w[c] += t[c];
  }
}

// Forward, one workgroup per (front, chunk of ND_CHUNK front rows); Q threads per row.
template <typename T, int TS, int XS, int Q>
__global__ __launch_bounds__(ND_CHUNK * Q) void k_nd_forward(nd_args<T> a, const int* __restrict__ cfront,
                                                             const int* __restrict__ crow0,
                                                             const double* __restrict__ in) {
  constexpr int GL = nd_group_log2<T>(), G = 1 << GL;
  constexpr int STG = TS >= 16 ? ND_STAGE / 2 : ND_STAGE;   // entries of w staged per round (32 KiB at 8 and 16 columns)
  __shared__ double ws[STG][TS];
  __shared__ double red[Q > 1 ? Q - 1 : 1][ND_CHUNK][TS];
  const int s = cfront[blockIdx.x], r0 = crow0[blockIdx.x], coff = blockIdx.y * TS;
  const int n = a.n[s], f = n + a.m[s], ld = a.ld[s];
  const T* __restrict__ P = a.F + a.offF[s];
  const int* __restrict__ rows = a.rows + a.rows_off[s];
  const int* __restrict__ src = a.src + 2 * (size_t)a.rows_off[s];
  const int cc0 = a.ccoff[2 * s], cc1 = a.ccoff[2 * s + 1];
  const int tid = threadIdx.x, rl = tid % ND_CHUNK, q = __builtin_amdgcn_readfirstlane(tid / ND_CHUNK);
  const int r = r0 + rl;
  const bool on = r < f;
  const int hi = min(r, n);                   // columns 0 .. hi - 1 of front row r
  const int gtot = (hi + G - 1) >> GL;
  const int jwg = min(n, r0 + ND_CHUNK);      // columns this workgroup meets
  const T* __restrict__ p = P + (on ? r : 0);
  T cf[G];
  int g = q;
  nd_dot_load<T, G>(cf, p, (size_t)ld, g, gtot, 0, hi, on);
  double acc[TS], own[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) { acc[c] = 0.0; own[c] = 0.0; }
  if (q == 0 && on && r >= n) nd_gather_w<TS, XS>(a, rows, src, cc0, cc1, r, n, in, coff, own);
  for (int c0 = 0; c0 < jwg; c0 += STG) {
    if (c0 > 0) __syncthreads();
    for (int jj = tid; jj < STG; jj += ND_CHUNK * Q) {
      double w[TS];
#pragma unroll
      for (int c = 0; c < TS; ++c) w[c] = 0.0;
      if (c0 + jj < jwg) nd_gather_w<TS, XS>(a, rows, src, cc0, cc1, c0 + jj, n, in, coff, w);
      double2* wq = reinterpret_cast<double2*>(ws[jj]);
#pragma unroll
      for (int c = 0; c < TS / 2; ++c) wq[c] = make_double2(w[2 * c], w[2 * c + 1]);
    }
    __syncthreads();
    if (q == 0 && on && r < n && r >= c0 && r < c0 + STG) {
#pragma unroll
      for (int c = 0; c < TS; ++c) own[c] = ws[r - c0][c];
    }
    nd_dot<TS, Q, STG>(acc, cf, p, (size_t)ld, g, min(gtot, (c0 + STG) >> GL), gtot, 0, hi, on, ws, c0);
  }
  if constexpr (Q > 1) {
    if (q > 0) {
#pragma unroll
      for (int c = 0; c < TS; ++c) red[q - 1][rl][c] = acc[c];
    }
    __syncthreads();
  }
  if (q == 0 && on) {
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      double sm = acc[c];
      if constexpr (Q > 1) {
#pragma unroll
        for (int k = 0; k < Q - 1; ++k) sm += red[k][rl][c];
      }
      own[c] += sm;
    }
    if (r < n) {
      const int gr = rows[r];
      const double id = a.dinv[gr];
#pragma unroll
      for (int c = 0; c < TS; ++c) own[c] *= id;
      store_row_s<TS, XS>(a.Y + coff, (size_t)gr, own);
    } else {
      store_row_s<TS, XS>(a.contrib + coff, (size_t)(a.coff[s] + r - n), own);
    }
  }
}

// Backward, one workgroup per (front, block of ND_COLS pivot columns); W wavefronts share the rows.
template <typename T, int TS, int XS, int W>
__global__ __launch_bounds__(64 * W) void k_nd_backward(nd_args<T> a, const int* __restrict__ cfront,
                                                        const int* __restrict__ ccol0, double* __restrict__ out) {
  constexpr int GL = nd_group_log2<T>(), G = 1 << GL;
  constexpr int NSTG = TS >= 16 ? 256 : TS >= 8 ? 512 : 1024;  // rows of v staged per round
  __shared__ double vs[NSTG][TS];
  __shared__ double red[W - 1][ND_COLS][TS];
  const int s = cfront[blockIdx.x], k0 = ccol0[blockIdx.x], coff = blockIdx.y * TS;
  const int n = a.n[s], f = n + a.m[s], ldb = PA_ND_LD(n);
  const T* __restrict__ U = a.B + a.offB[s];
  const int* __restrict__ rows = a.rows + a.rows_off[s];
  const int tid = threadIdx.x, kk = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = k0 + kk;
  const bool on = k < n;
  const int gtot = (f + G - 1) >> GL;
  const T* __restrict__ p = U + (on ? k : 0);
  T cf[G];
  int g = (k0 >> GL) + q;                     // (k0: a multiple of ND_COLS, so of G)
  nd_dot_load<T, G>(cf, p, (size_t)ldb, g, gtot, k + 1, f, on);
  double acc[TS], own[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) { acc[c] = 0.0; own[c] = 0.0; }
  for (int c0 = k0; c0 < f; c0 += NSTG) {
    if (c0 > k0) __syncthreads();
    for (int ii = tid; ii < NSTG; ii += 64 * W) {
      const int i = c0 + ii;
      double v[TS];
#pragma unroll
      for (int c = 0; c < TS; ++c) v[c] = 0.0;
      if (i < f) {
        const int gr = rows[i];
        if (i < n) {
          load_row_s<TS, XS>(a.Y + coff, (size_t)gr, v);
          const double id = a.dinv[gr];
#pragma unroll
          for (int c = 0; c < TS; ++c) v[c] *= id;
        } else {
          load_row_s<TS, XS>(out + coff, (size_t)gr, v);
        }
      }
      double2* vq = reinterpret_cast<double2*>(vs[ii]);
#pragma unroll
      for (int c = 0; c < TS / 2; ++c) vq[c] = make_double2(v[2 * c], v[2 * c + 1]);
    }
    __syncthreads();
    if (q == 0 && on && k >= c0 && k < c0 + NSTG) {
#pragma unroll
      for (int c = 0; c < TS; ++c) own[c] = vs[k - c0][c];
    }
    nd_dot<TS, W, NSTG>(acc, cf, p, (size_t)ldb, g, min(gtot, (c0 + NSTG) >> GL), gtot, k + 1, f, on, vs, c0);
  }
  if (q > 0) {
#pragma unroll
    for (int c = 0; c < TS; ++c) red[q - 1][kk][c] = acc[c];
  }
  __syncthreads();
  if (q == 0 && on) {
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      double sm = acc[c];
#pragma unroll
      for (int j = 0; j < W - 1; ++j) sm += red[j][kk][c];
      own[c] += sm;
    }
    store_row_s<TS, XS>(out + coff, (size_t)rows[k], own);
  }
}

// dst[i] = src[i] rounded to the nearest float, i < n (grid-stride)
__global__ __launch_bounds__(WG) void k_nd_round(size_t n, const double* __restrict__ src, float* __restrict__ dst) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) dst[i] = __double2float_rn(src[i]);
}

}  // namespace

// 16-column panels: all columns in one pass over the factor (172 VGPRs, two wavefronts per SIMD: 2.6 TB/s
// of factor bytes) instead of two 8-column passes at 4.5 TB/s each: 4.37 against 5.09 ms per apply on the
// 64-block elasticity problem (round 3, same-call A/B).
// one level of the tree; launches of few workgroups put more threads on each output
template <typename T, int XS>
static int nd_launch_fwd(const nd_args<T>& a, const int* cfront, const int* crow0, int nwg, const double* in) {
  if (nwg <= 0) return 0;
  constexpr int few = 1024;
  if constexpr (XS == 16) {                   // all 16 columns in one pass over the factor
    if (nwg < few) PA_LAUNCH((k_nd_forward<T, 16, 16, 2>), dim3(nwg), dim3(ND_CHUNK * 2), 0, cur_stream(), a, cfront, crow0, in);
    else PA_LAUNCH((k_nd_forward<T, 16, 16, 1>), dim3(nwg), dim3(ND_CHUNK), 0, cur_stream(), a, cfront, crow0, in);
    return kfail("k_nd_forward");
  }
  constexpr int TS = XS <= 8 ? XS : 8;
  constexpr int QB = TS >= 8 ? 2 : 4;
  const dim3 grid(nwg, XS / TS);
  if (nwg < few) PA_LAUNCH((k_nd_forward<T, TS, XS, QB>), grid, dim3(ND_CHUNK * QB), 0, cur_stream(), a, cfront, crow0, in);
  else PA_LAUNCH((k_nd_forward<T, TS, XS, 1>), grid, dim3(ND_CHUNK), 0, cur_stream(), a, cfront, crow0, in);
  return kfail("k_nd_forward");
}

template <typename T, int XS>
static int nd_launch_bwd(const nd_args<T>& a, const int* cfront, const int* ccol0, int nwg, double* out) {
  if (nwg <= 0) return 0;
  constexpr int few = 2048;
  if constexpr (XS == 16) {
    PA_LAUNCH((k_nd_backward<T, 16, 16, 4>), dim3(nwg), dim3(256), 0, cur_stream(), a, cfront, ccol0, out);
    return kfail("k_nd_backward");
  }
  constexpr int TS = XS <= 8 ? XS : 8;
  constexpr int WB = TS >= 8 ? 8 : 16;
  const dim3 grid(nwg, XS / TS);
  if (nwg < few) PA_LAUNCH((k_nd_backward<T, TS, XS, WB>), grid, dim3(64 * WB), 0, cur_stream(), a, cfront, ccol0, out);
  else PA_LAUNCH((k_nd_backward<T, TS, XS, 4>), grid, dim3(256), 0, cur_stream(), a, cfront, ccol0, out);
  return kfail("k_nd_backward");
}

// levels are listed bottom-up: forward in that order, backward reversed
template <typename T>
static int nd_apply(const pa_nd_plan_t* pl, const T* F, const T* B, int ts, const double* in, double* out) {
  nd_args<T> a{pl->n, pl->m, pl->ld, pl->offF, pl->offB, pl->rows_off, pl->coff, pl->ccoff, pl->rows, pl->src,
               pl->dinv, F, B, pl->contrib, pl->Y};
  for (int i = 0; i < pl->nlevel; ++i) {
    int rc = 0;
    TS_DISPATCH(ts, rc = (nd_launch_fwd<T, TS_>(a, pl->f_front[i], pl->f_row0[i], pl->f_count[i], in)));
    if (rc) return rc;
  }
  for (int i = pl->nlevel - 1; i >= 0; --i) {
    int rc = 0;
    TS_DISPATCH(ts, rc = (nd_launch_bwd<T, TS_>(a, pl->b_front[i], pl->b_col0[i], pl->b_count[i], out)));
    if (rc) return rc;
  }
  return 0;
}

extern "C" {

int pa_nd_chunk_rows(void) { return ND_CHUNK; }
int pa_nd_block_cols(void) { return ND_COLS; }

int pa_k_nd_apply(const pa_nd_plan_t* pl, int ts, const double* in, double* out) {
  if (pl->F32) return nd_apply<float>(pl, pl->F32, pl->B32, ts, in, out);
  return nd_apply<double>(pl, pl->F, pl->B, ts, in, out);
}

int pa_k_nd_round(const double* src, float* dst, size_t n) {
  if (n == 0) return 0;
  const size_t want = (n + WG - 1) / WG;
  PA_LAUNCH(k_nd_round, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(WG), 0, cur_stream(), n, src, dst);
  return kfail("k_nd_round");
}

}  // extern "C"
