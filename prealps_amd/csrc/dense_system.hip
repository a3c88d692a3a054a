// dense_system.hip -- the caller's own system around the ECG block iteration (preAlps_ECGSolveSystem): the gather of
// B and X0 from the caller's order and units into the staging arrays of the start, the scatter of the solutions back,
// and the per-system residual norms in the caller's units (on several processes: folded behind the words a collective of
// the iteration carries, k_sys_norms_ride), with their C launchers (pa_device.h).  The iteration works
// on A' = P D A D P^T; local row i is the caller's row src[i] and dl[i] = d[src[i]] its scaling factor (1.0 when the
// operator is unscaled), so b' = dl * b[src], x0' = x0[src] / dl, x[src] = dl * x' and r[src] = r' / dl.
// See dense_gram.hip for the layout of panels.
#include "dense_device.h"

namespace {

// Bp(i, j) = dl[i] * B(src[i], j) and, with a guess, X0p(i, j) = X0(src[i], j) / dl[i] (a true division: the bits of
// NumPy's x0 / d), both column major with leading dimension m.  Each workgroup leaves the sums of B(src[i], j)^2 over
// its rows in sums[blk*TS + j], the layout of k_colnorm2, for k_group_norms with s = 1: the caller's ||b_j||^2.  The
// reads of B and X0 follow the permutation (8 bytes each, a gather); everything else streams.
template <int TS>
__global__ __launch_bounds__(WG) void k_sys_gather(int m, int k, const int* __restrict__ src,
                                                   const double* __restrict__ dl, const double* __restrict__ B, size_t ldb,
                                                   const double* __restrict__ X0, size_t ldx0, double* __restrict__ Bp,
                                                   double* __restrict__ X0p, double* __restrict__ sums) {
  double acc[TS];
#pragma unroll
  for (int j = 0; j < TS; ++j) acc[j] = 0.0;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    const size_t from = (size_t)src[row];
    const double d = dl[row];
#pragma unroll
    for (int j = 0; j < TS; ++j)
      if (j < k) {
        const double b = B[from + (size_t)j * ldb];
        Bp[row + (size_t)j * m] = d * b;
        acc[j] = fma(b, b, acc[j]);
        if (X0) X0p[row + (size_t)j * m] = X0[from + (size_t)j * ldx0] / d;
      }
  }
  block_sum_cols<TS>(acc, sums + (size_t)blockIdx.x * TS);
}

// Xout(src[i], j) = dl[i] * (the sum of the columns of system j of X, added in ascending c as k_rowsum_groups and
// k_rowsum add them).
template <int TS>
__global__ __launch_bounds__(WG) void k_sys_scatter(int m, int k, int s, const double* __restrict__ X,
                                                    const int* __restrict__ src, const double* __restrict__ dl,
                                                    double* __restrict__ Xout, size_t ldx) {
  const int nc = k * s;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double x[TS];
    load_row<TS>(X, row, x);
    const size_t to = (size_t)src[row];
    const double d = dl[row];
    double acc = 0.0;
    int j = 0, cnt = 0;
#pragma unroll
    for (int c = 0; c < TS; ++c)
      if (c < nc) {
        acc += x[c];
        if (++cnt == s) { Xout[to + (size_t)j * ldx] = d * acc; acc = 0.0; cnt = 0; ++j; }
      }
  }
}

// The per-system residual norms in the caller's units: the sum of a system's columns of R is that system's whole
// recurrence residual in the scaled space, and divided by dl it is b_j - A x_j at the caller's row.  Each workgroup
// leaves its share of sum_i ((sum_c R(i, j*s + c)) / dl[i])^2 in part[blk*TS + j] for k_group_norms with s = 1.  One
// read of the R panel and of dl: 8 m (TS + 1) bytes.
template <int TS>
__global__ __launch_bounds__(WG) void k_sys_norms(int m, int k, int s, const double* __restrict__ R,
                                                  const double* __restrict__ dl, double* __restrict__ part) {
  double acc[TS];
#pragma unroll
  for (int j = 0; j < TS; ++j) acc[j] = 0.0;
  const int nc = k * s;
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    double r[TS];
    load_row<TS>(R, row, r);
    const double d = dl[row];
    // a running sum up to the last column of each system, ascending as k_rowsum_groups adds them
    double run = 0.0;
    int j = 0, cnt = 0;
#pragma unroll
    for (int c = 0; c < TS; ++c)
      if (c < nc) {
        run += r[c];
        if (++cnt == s) {
          const double v = run / d;
#pragma unroll
          for (int q = 0; q < TS; ++q) acc[q] = (q == j) ? fma(v, v, acc[q]) : acc[q];      // (registers: no run-time index)
          run = 0.0; cnt = 0; ++j;
        }
      }
  }
  block_sum_cols<TS>(acc, part + (size_t)blockIdx.x * TS);
}

// Xout(src[i], j) = Xin(src[i], j): the rows this process owns of a guess that is already the answer, bit for bit.
__global__ __launch_bounds__(WG) void k_sys_copy_rows(int m, int k, const int* __restrict__ src, const double* __restrict__ Xin,
                                                      size_t ldin, double* __restrict__ Xout, size_t ldout) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t row = (size_t)blockIdx.x * WG + threadIdx.x; row < (size_t)m; row += stride) {
    const size_t at = (size_t)src[row];
    for (int j = 0; j < k; ++j) Xout[at + (size_t)j * ldout] = Xin[at + (size_t)j * ldin];
  }
}

// The caller's metric on several processes: the sums are this process's share, so -- as k_group_norms_ride does for
// several systems -- they go behind the two words a collective of the iteration carries anyway.  buf[0] = the local
// scaled sum of squares of all of R, folded from rtr group by group with the groups added in ascending j (the
// additions of k_group_norms_ride, so the same bits), buf[1] = the Cholesky status, buf[2 + j] = the fold of the
// partial sums k_sys_norms left (one column per system, s = 1): system j's share of ||b_j - A x_j||^2 in the caller's
// units.  One workgroup; nothing else is written.
__global__ __launch_bounds__(WG) void k_sys_norms_ride(const double* __restrict__ rtr, int rtr_nblk,
                                                       const double* __restrict__ sys, int sys_nblk, int ts, int k, int s,
                                                       const int* __restrict__ info, double* __restrict__ buf) {
  __shared__ double red[WG];
  __shared__ double grp[16];
  const double g = group_fold(rtr, rtr_nblk, ts, k, s, red);
  if (threadIdx.x < k) grp[threadIdx.x] = g;
  __syncthreads();      // (grp is complete, and red has been read: the second fold may write it)
  const double o = group_fold(sys, sys_nblk, ts, k, 1, red);
  if (threadIdx.x < k) buf[2 + threadIdx.x] = o;
  if (threadIdx.x == 0) {
    double all = 0.0;
    for (int j = 0; j < k; ++j) all += grp[j];
    buf[0] = all;
    buf[1] = info ? (double)info[0] : 0.0;
  }
}

}  // namespace

extern "C" {

static int sys_args_bad(const char* what, int m, int ts, int k, int s) {
  if (m >= 0 && k >= 1 && s >= 1 && k * s <= ts && ts <= 16) return 0;
  pa_rt_set_error("%s: %d systems of %d columns do not fit a panel of stride %d (%d rows)", what, k, s, ts, m);
  return 1;
}

int pa_k_sys_gather(int m, int ts, int k, const int* src, const double* dl, const double* B, int ldb, const double* X0,
                    int ldx0, double* Bp, double* X0p, double* sums, int* nblk) {
  if (sys_args_bad("pa_k_sys_gather", m, ts, k, 1)) return 1;
  if (ldb < m || (X0 && (ldx0 < m || !X0p))) {
    pa_rt_set_error("pa_k_sys_gather: leading dimensions %d / %d below the %d rows", ldb, ldx0, m);
    return 1;
  }
  const int blocks = update_grid(m, 4);
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_sys_gather<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m, k, src, dl, B, (size_t)ldb,
                            X0, (size_t)ldx0, Bp, X0p, sums));
  return kfail("k_sys_gather");
}

int pa_k_sys_scatter(int m, int ts, int k, int s, const double* X, const int* src, const double* dl, double* Xout,
                     int ldx) {
  if (sys_args_bad("pa_k_sys_scatter", m, ts, k, s)) return 1;
  if (ldx < m) { pa_rt_set_error("pa_k_sys_scatter: leading dimension %d below the %d rows", ldx, m); return 1; }
  TS_DISPATCH(ts, PA_LAUNCH((k_sys_scatter<TS_>), dim3(update_grid(m, 4)), dim3(WG), 0, cur_stream(), m, k, s, X, src,
                            dl, Xout, (size_t)ldx));
  return kfail("k_sys_scatter");
}

int pa_k_sys_norms(int m, int ts, int k, int s, const double* R, const double* dl, double* part, int* nblk) {
  if (sys_args_bad("pa_k_sys_norms", m, ts, k, s)) return 1;
  const int blocks = update_grid(m, 4);
  *nblk = blocks;
  TS_DISPATCH(ts, PA_LAUNCH((k_sys_norms<TS_>), dim3(blocks), dim3(WG), 0, cur_stream(), m, k, s, R, dl, part));
  return kfail("k_sys_norms");
}

int pa_k_sys_copy_rows(int m, int k, const int* src, const double* Xin, int ldin, double* Xout, int ldout) {
  if (m < 0 || k < 1 || !src || !Xin || !Xout || ldin < m || ldout < m) {
    pa_rt_set_error("pa_k_sys_copy_rows: %d rows of %d columns, leading dimensions %d / %d", m, k, ldin, ldout);
    return 1;
  }
  PA_LAUNCH(k_sys_copy_rows, dim3(update_grid(m, 4)), dim3(WG), 0, cur_stream(), m, k, src, Xin, (size_t)ldin, Xout,
            (size_t)ldout);
  return kfail("k_sys_copy_rows");
}

int pa_k_sys_norms_ride(const double* rtr_part, int rtr_nblk, const double* sys_part, int sys_nblk, int ts, int k, int s,
                        const int* info, double* buf) {
  if (sys_args_bad("pa_k_sys_norms_ride", 0, ts, k, s)) return 1;
  if (!buf || !rtr_part || !sys_part || rtr_nblk < 0 || sys_nblk < 0) {
    pa_rt_set_error("pa_k_sys_norms_ride: no buffer for the %d sums, or no partial sums to fold", k);
    return 1;
  }
  PA_LAUNCH(k_sys_norms_ride, dim3(1), dim3(WG), 0, cur_stream(), rtr_part, rtr_nblk, sys_part, sys_nblk, ts, k, s, info,
            buf);
  return kfail("k_sys_norms_ride");
}

}  // extern "C"
