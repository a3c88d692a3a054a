// coarse.hip -- the coarse correction of the two-level block-Jacobi preconditioner on the device:
// out += Z Einv Z^T in (pa_device.h: pa_coarse_plan_t, pa_k_coarse_apply).  fp64 throughout, on the library
// stream.  All of it is bandwidth work: two passes over a panel (in, then out read-modify-write), one over the
// m x k array zv each, and one streaming pass over the nc x nc inverse.  No atomics: every sum has one fixed
// order (lane, wavefront, workgroup, chunk list), so two applies of the same input agree in bits.
// Several processes: the coarse vector is summed over the ranks between the gather and the product with the inverse,
// of which a rank keeps the rows its own aggregates need (k_coarse_einv_rows).
#include "kernels_common.h"

namespace {

constexpr int CO_MAXK = 8;     // vectors per aggregate at most (PA_COARSE_MAX_VECS)
constexpr int CO_RB = 4;       // rows of Einv per workgroup of k_coarse_einv

// A workgroup of 256 lanes covers 256 / (TS / 2) panel rows per pass: lane = (row, column pair), 16 bytes per
// lane, consecutive lanes at consecutive addresses.
template <int TS>
__global__ __launch_bounds__(WG) void k_coarse_restrict(int k, int ncols, const double* __restrict__ zv,
                                                        const int* __restrict__ ch_row0, const int* __restrict__ ch_nrows,
                                                        const double* __restrict__ in, double* __restrict__ partial) {
  constexpr int CP = TS / 2, RP = WG / CP;
  __shared__ double red[WG / 64][CO_MAXK][TS];
  const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cp = tid % CP, rsub = tid / CP;
  const int r0 = ch_row0[ch], nr = ch_nrows[ch];
  const bool live0 = 2 * cp < ncols, live1 = 2 * cp + 1 < ncols;
  double acc[CO_MAXK][2];
#pragma unroll
  for (int a = 0; a < CO_MAXK; ++a) acc[a][0] = acc[a][1] = 0.0;
  for (int r = rsub; r < nr; r += RP) {
    const size_t i = (size_t)(r0 + r);
    const double2 v = *reinterpret_cast<const double2*>(in + i * TS + 2 * cp);
    const double x0 = live0 ? v.x : 0.0, x1 = live1 ? v.y : 0.0;      // dead columns may hold anything
    const double* z = zv + i * k;
#pragma unroll
    for (int a = 0; a < CO_MAXK; ++a)
      if (a < k) { const double za = z[a]; acc[a][0] += za * x0; acc[a][1] += za * x1; }
  }
  // lanes of one column pair are CP apart: fold the wavefront, then the four wavefronts through LDS
#pragma unroll
  for (int a = 0; a < CO_MAXK; ++a)
    if (a < k) {
#pragma unroll
      for (int off = 32; off >= CP; off >>= 1) {
        acc[a][0] += __shfl_xor(acc[a][0], off, 64);
        acc[a][1] += __shfl_xor(acc[a][1], off, 64);
      }
      if (lane < CP) { red[wave][a][2 * cp] = acc[a][0]; red[wave][a][2 * cp + 1] = acc[a][1]; }
    }
  __syncthreads();
  if (tid < k * TS) {
    const int a = tid / TS, c = tid % TS;
    partial[((size_t)ch * k + a) * TS + c] = ((red[0][a][c] + red[1][a][c]) + red[2][a][c]) + red[3][a][c];
  }
}

// c[g*k + a][cc] = the sum of aggregate g's chunk partials, in list order; one lane per entry
__global__ __launch_bounds__(WG) void k_coarse_gather(int k, int ts, int nc, const int* __restrict__ agg_ptr,
                                                      const int* __restrict__ agg_chunk, const double* __restrict__ partial,
                                                      double* __restrict__ c) {
  const int idx = blockIdx.x * WG + threadIdx.x;
  if (idx >= nc * ts) return;
  const int row = idx / ts, cc = idx % ts, g = row / k, a = row % k;
  double s = 0.0;
  for (int x = agg_ptr[g]; x < agg_ptr[g + 1]; ++x) s += partial[((size_t)agg_chunk[x] * k + a) * ts + cc];
  c[idx] = s;
}

// y = Einv c: a workgroup owns CO_RB rows of Einv and streams them once, lane j of a pass holding row j of c in
// registers (c, nc x TS, is the tile: it is read once per workgroup, from L2).  Einv is read coalesced, 8 bytes
// per lane.
template <int TS>
__global__ __launch_bounds__(WG) void k_coarse_einv(int nc, const double* __restrict__ Einv, const double* __restrict__ c,
                                                    double* __restrict__ y) {
  __shared__ double red[WG / 64][CO_RB][TS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * CO_RB;
  double acc[CO_RB][TS];
#pragma unroll
  for (int rr = 0; rr < CO_RB; ++rr)
#pragma unroll
    for (int cc = 0; cc < TS; ++cc) acc[rr][cc] = 0.0;
  for (int j = tid; j < nc; j += WG) {
    double cj[TS];
    load_row<TS>(c, (size_t)j, cj);
#pragma unroll
    for (int rr = 0; rr < CO_RB; ++rr) {
      const double e = r0 + rr < nc ? Einv[(size_t)(r0 + rr) * nc + j] : 0.0;
#pragma unroll
      for (int cc = 0; cc < TS; ++cc) acc[rr][cc] += e * cj[cc];
    }
  }
#pragma unroll
  for (int rr = 0; rr < CO_RB; ++rr)
#pragma unroll
    for (int cc = 0; cc < TS; ++cc) {
      double v = acc[rr][cc];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) red[wave][rr][cc] = v;
    }
  __syncthreads();
  if (tid < CO_RB * TS) {
    const int rr = tid / TS, cc = tid % TS;
    if (r0 + rr < nc) y[(size_t)(r0 + rr) * TS + cc] = ((red[0][rr][cc] + red[1][rr][cc]) + red[2][rr][cc]) + red[3][rr][cc];
  }
}

// y[rows[x]] = slab[x] . c for the nrows listed rows of the inverse (several processes: a rank keeps the rows its own
// aggregates need).  k_coarse_einv with a row list: a workgroup owns CO_RB consecutive entries of the list and streams
// their slab rows once, 8 bytes per lane, coalesced; the fold is the same -- lane, wavefront, the four wavefronts
// through LDS in a fixed order -- so a row's sum has one order.  Rows of y outside the list are not written.
template <int TS>
__global__ __launch_bounds__(WG) void k_coarse_einv_rows(int nc, int nrows, const int* __restrict__ rows,
                                                         const double* __restrict__ slab, const double* __restrict__ c,
                                                         double* __restrict__ y) {
  __shared__ double red[WG / 64][CO_RB][TS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * CO_RB;
  double acc[CO_RB][TS];
#pragma unroll
  for (int rr = 0; rr < CO_RB; ++rr)
#pragma unroll
    for (int cc = 0; cc < TS; ++cc) acc[rr][cc] = 0.0;
  for (int j = tid; j < nc; j += WG) {
    double cj[TS];
    load_row<TS>(c, (size_t)j, cj);
#pragma unroll
    for (int rr = 0; rr < CO_RB; ++rr) {
      const double e = x0 + rr < nrows ? slab[(size_t)(x0 + rr) * nc + j] : 0.0;
#pragma unroll
      for (int cc = 0; cc < TS; ++cc) acc[rr][cc] += e * cj[cc];
    }
  }
#pragma unroll
  for (int rr = 0; rr < CO_RB; ++rr)
#pragma unroll
    for (int cc = 0; cc < TS; ++cc) {
      double v = acc[rr][cc];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) red[wave][rr][cc] = v;
    }
  __syncthreads();
  if (tid < CO_RB * TS) {
    const int rr = tid / TS, cc = tid % TS;
    if (x0 + rr < nrows)
      y[(size_t)rows[x0 + rr] * TS + cc] = ((red[0][rr][cc] + red[1][rr][cc]) + red[2][rr][cc]) + red[3][rr][cc];
  }
}

// out[i][c] += sum_a zv[i][a] y[g*k + a][c] over the rows of the chunk, the lane layout of k_coarse_restrict
template <int TS>
__global__ __launch_bounds__(WG) void k_coarse_prolong_add(int k, int ncols, const double* __restrict__ zv,
                                                           const int* __restrict__ ch_row0, const int* __restrict__ ch_nrows,
                                                           const int* __restrict__ ch_aggr, const double* __restrict__ y,
                                                           double* __restrict__ out) {
  constexpr int CP = TS / 2, RP = WG / CP;
  const int ch = blockIdx.x, tid = threadIdx.x;
  const int cp = tid % CP, rsub = tid / CP;
  const int r0 = ch_row0[ch], nr = ch_nrows[ch], g = ch_aggr[ch];
  const bool live0 = 2 * cp < ncols, live1 = 2 * cp + 1 < ncols;
  double yv[CO_MAXK][2];
#pragma unroll
  for (int a = 0; a < CO_MAXK; ++a) {
    yv[a][0] = yv[a][1] = 0.0;
    if (a < k) {
      const double2 v = *reinterpret_cast<const double2*>(y + ((size_t)g * k + a) * TS + 2 * cp);
      yv[a][0] = v.x; yv[a][1] = v.y;
    }
  }
  for (int r = rsub; r < nr; r += RP) {
    const size_t i = (size_t)(r0 + r);
    const double* z = zv + i * k;
    double2* po = reinterpret_cast<double2*>(out + i * TS + 2 * cp);
    double2 o = *po;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int a = 0; a < CO_MAXK; ++a)
      if (a < k) { const double za = z[a]; s0 += za * yv[a][0]; s1 += za * yv[a][1]; }
    if (live0) o.x += s0;
    if (live1) o.y += s1;
    *po = o;
  }
}

}  // namespace

extern "C" int pa_allreduce(double* dev_buf, int count);     // pa_host.h: the sum over the processes, on the library stream

extern "C" int pa_k_coarse_einv_rows(int nc, int nrows, const int* rows, const double* slab, const double* c, double* y, int ts) {
  if (!rows || !slab || !c || !y) {
    pa_rt_set_error("pa_k_coarse_einv_rows: wrong test 'rows != NULL && slab != NULL && c != NULL && y != NULL'");
    return 1;
  }
  if (nc < 1 || nrows < 1 || nrows > nc) {
    pa_rt_set_error("pa_k_coarse_einv_rows: %d rows of %d coarse unknowns", nrows, nc);
    return 1;
  }
  TS_DISPATCH(ts, PA_LAUNCH(k_coarse_einv_rows<TS_>, dim3((nrows + CO_RB - 1) / CO_RB), dim3(WG), 0, cur_stream(), nc, nrows,
                            rows, slab, c, y));
  return kfail("k_coarse_einv_rows");
}

extern "C" int pa_k_coarse_apply(const pa_coarse_plan_t* pl, int ts, int ncols, const double* in, double* out) {
  if (!pl || !pl->zv || !pl->Einv || !pl->partial || !pl->c || !pl->y || pl->nchunks <= 0 || pl->nc <= 0 ||
      pl->k < 1 || pl->k > CO_MAXK || pl->nc != pl->naggr * pl->k) {
    pa_rt_set_error("pa_k_coarse_apply: no coarse space");
    return 1;
  }
  if (!in || !out || ncols < 1 || ncols > ts) {
    pa_rt_set_error("pa_k_coarse_apply: %d columns at panel stride %d", ncols, ts);
    return 1;
  }
  const int k = pl->k, nc = pl->nc;
  TS_DISPATCH(ts, PA_LAUNCH(k_coarse_restrict<TS_>, dim3(pl->nchunks), dim3(WG), 0, cur_stream(), k, ncols, pl->zv,
                            pl->ch_row0, pl->ch_nrows, in, pl->partial));
  if (kfail("k_coarse_restrict")) return 1;
  PA_LAUNCH(k_coarse_gather, dim3((nc * ts + WG - 1) / WG), dim3(WG), 0, cur_stream(), k, ts, nc, pl->agg_ptr,
            pl->agg_chunk, pl->partial, pl->c);
  if (kfail("k_coarse_gather")) return 1;
  if (pl->rows) {      // several processes: c summed over the ranks, then the rank's own rows of the inverse
    if (pa_allreduce(pl->c, nc * ts)) {
      pa_rt_set_error("pa_k_coarse_apply: the all-reduce of the %d x %d coarse vector failed", nc, ts);
      return 1;
    }
    if (pa_k_coarse_einv_rows(nc, pl->nrows, pl->rows, pl->Einv, pl->c, pl->y, ts)) return 1;
  } else {
    TS_DISPATCH(ts, PA_LAUNCH(k_coarse_einv<TS_>, dim3((nc + CO_RB - 1) / CO_RB), dim3(WG), 0, cur_stream(), nc, pl->Einv,
                              pl->c, pl->y));
    if (kfail("k_coarse_einv")) return 1;
  }
  TS_DISPATCH(ts, PA_LAUNCH(k_coarse_prolong_add<TS_>, dim3(pl->nchunks), dim3(WG), 0, cur_stream(), k, ncols, pl->zv,
                            pl->ch_row0, pl->ch_nrows, pl->ch_aggr, pl->y, out));
  return kfail("k_coarse_prolong_add");
}
