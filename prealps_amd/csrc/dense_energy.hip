// dense_energy.hip -- the energy-norm drops of one block CG iteration (ecg_energy.h): with A-orthonormal directions
// the update X += P alpha takes delta_j = || alpha 1_{G_j} ||_2^2 off the squared energy error of system j, G_j its
// columns j*s .. j*s + s - 1 of the rows x T block alpha.  One small workgroup reads the alpha the update of X uses and
// leaves the k drops in a device slot and in pinned host words; the host reads them with the residual norm.
#include "dense_device.h"

namespace {

// alpha: rows x T, column major, leading dimension ld (rows, T <= 16).  Thread (j, r) = (tid >> 4, tid & 15) forms
// v_r = sum_{c in G_j} alpha(r, c) in ascending c; thread j then adds v_r^2 in ascending r.  Every sum has one fixed
// order and nothing is accumulated across threads, so two launches on the same alpha agree in bits.  No atomics.
__global__ __launch_bounds__(WG) void k_energy_drops(const double* __restrict__ alpha, int rows, int ld, int k, int s,
                                                     double* __restrict__ out, double* __restrict__ host) {
  __shared__ double v[16][16];
  const int j = threadIdx.x >> 4, r = threadIdx.x & 15;
  double acc = 0.0;
  if (j < k && r < rows) {
    const double* col = alpha + (size_t)(j * s) * ld + r;
    for (int c = 0; c < s; ++c) acc += col[(size_t)c * ld];
  }
  v[j][r] = acc;      // (rows beyond the block hold 0, and are not read)
  __syncthreads();
  if (threadIdx.x < k) {
    double d = 0.0;
    for (int q = 0; q < rows; ++q) d = fma(v[threadIdx.x][q], v[threadIdx.x][q], d);
    out[threadIdx.x] = d;
    if (host) __hip_atomic_store(host + threadIdx.x, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (host) __threadfence_system();
}

}  // namespace

extern "C" {

int pa_k_energy_drops(const double* alpha, int rows, int ld, int T, int k, int s, double* out, double* host) {
  if (!alpha || !out) { pa_rt_set_error("pa_k_energy_drops: no alpha, or no place for the %d drops", k); return 1; }
  if (rows < 1 || rows > 16 || T < 1 || T > 16 || ld < rows) {
    pa_rt_set_error("pa_k_energy_drops: alpha of %d x %d with leading dimension %d (1 .. 16 rows and columns, ld >= rows)",
                    rows, T, ld);
    return 1;
  }
  if (k < 1 || s < 1 || k * s > T) {
    pa_rt_set_error("pa_k_energy_drops: %d systems of %d columns do not fit the %d columns of alpha", k, s, T);
    return 1;
  }
  PA_LAUNCH(k_energy_drops, dim3(1), dim3(WG), 0, cur_stream(), alpha, rows, ld, k, s, out, host);
  return kfail("k_energy_drops");
}

}  // extern "C"
