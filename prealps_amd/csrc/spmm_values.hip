// spmm_values.hip -- new values for the SpMM plan that is on the device (preAlps_OperatorUpdateValues): the plan's
// value array is a fixed gather of the panel's values (spmm_plan.h: pa_spmm_plan_value_map), so an update of the
// matrix with the same pattern rewrites that one array in place and leaves slices, slots and blocks alone.
#include "kernels_common.h"

namespace {

// val[s] = map[s] ? pv[map[s] - 1] : 0.0 for the n stored slots (n even: every slot array of the three plans is a
// multiple of 64 long).  A streaming kernel: a lane takes two neighbouring slots -- one 8-byte load of the map, one
// 16-byte store -- and the grid strides over the pairs; val is written once and read by the next product at the
// earliest, hence the nontemporal hint.  The reads of pv follow the plan's slice order: entry-major inside a slice,
// so neighbouring lanes read neighbouring rows of the panel (a row apart in pv) and a slice's part of pv is read
// whole within a few steps, out of L2.
typedef unsigned u2v __attribute__((ext_vector_type(2)));
typedef double d2v __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(WG) void k_plan_set_values(const u2v* __restrict__ map, const double* __restrict__ pv,
                                                       double* __restrict__ val, size_t npairs) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < npairs; i += stride) {
    const u2v e = __builtin_nontemporal_load(map + i);
    d2v v;
    v.x = e.x ? pv[e.x - 1u] : 0.0;
    v.y = e.y ? pv[e.y - 1u] : 0.0;
    __builtin_nontemporal_store(v, reinterpret_cast<d2v*>(val) + i);
  }
}

// The packed run plan (spmm_pack.h): slot s of the unpacked array is lane s % 64 of position (s / 64) % 3 of step
// s / 192; its place in the packed array follows from the step's four words.  WRITE = false only counts the slots
// that would need a place the pack does not have (the caller then packs anew), so that nothing is written before
// the update is known to fit.
template <bool WRITE>
__global__ __launch_bounds__(WG) void k_pack_set_values(const unsigned* __restrict__ map, const double* __restrict__ pv,
                                                       const unsigned long long* __restrict__ meta,
                                                       double* __restrict__ packed, size_t n, unsigned* __restrict__ misses) {
  const size_t stride = (size_t)gridDim.x * WG;
  unsigned miss = 0;
  for (size_t s = (size_t)blockIdx.x * WG + threadIdx.x; s < n; s += stride) {
    const unsigned e = map[s];
    const double v = e ? pv[e - 1u] : 0.0;
    const size_t g = s / 192;
    const int p = (int)((s >> 6) % 3), lane = (int)(s & 63);
    const unsigned long long* __restrict__ q = meta + 4 * g;
    const unsigned long long mk = q[p];
    if ((mk >> lane) & 1ull) {
      if constexpr (WRITE) {
        size_t at = (size_t)q[3] + 1 + __popcll(mk & ((1ull << lane) - 1ull));
        if (p > 0) at += __popcll(q[0]);
        if (p > 1) at += __popcll(q[1]);
        packed[at] = v;
      }
    } else if (__double_as_longlong(v) != 0) ++miss;
  }
  if constexpr (!WRITE) { if (miss) atomicAdd(misses, miss); }
}

// The fp32 copy of a packed value array (preAlps_hip_set_operator_precision(32)): val32[i] = (float)val[i] for the n
// elements, the steps' zeros and the slack included (they stay 0.0f), so the masks and offsets of the pack address
// both arrays.  A streaming kernel, the grid strides over the elements.  A value that is finite in fp64 and rounds to
// +-Inf is counted (bad[0]) and one such value is left in bad[1]: the caller refuses the copy.
__global__ __launch_bounds__(WG) void k_plan_round_values(const double* __restrict__ val, float* __restrict__ val32,
                                                         size_t n, unsigned long long* __restrict__ bad) {
  const size_t stride = (size_t)gridDim.x * WG;
  unsigned lost = 0;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += stride) {
    const double v = __builtin_nontemporal_load(val + i);
    const float f = (float)v;
    __builtin_nontemporal_store(f, val32 + i);
    if (v - v == 0.0 && !(f - f == 0.0f)) { ++lost; bad[1] = (unsigned long long)__double_as_longlong(v); }
  }
  if (lost) atomicAdd(bad, (unsigned long long)lost);
}

}  // namespace

extern "C" int pa_k_plan_round_values(const double* val, float* val32, size_t n, unsigned long long* bad) {
  if (n == 0) return 0;
  const int cus = pa_rt_num_cus() > 0 ? pa_rt_num_cus() : 256;
  size_t blocks = (n + WG - 1) / WG;
  if (blocks > (size_t)8 * cus) blocks = (size_t)8 * cus;
  PA_LAUNCH(k_plan_round_values, dim3((unsigned)blocks), dim3(WG), 0, cur_stream(), val, val32, n, bad);
  return kfail("k_plan_round_values");
}

extern "C" int pa_k_pack_set_values(const unsigned* map, const double* pv, const unsigned long long* meta, double* packed,
                                    size_t n, int write, unsigned* misses) {
  if (n == 0) return 0;
  const int cus = pa_rt_num_cus() > 0 ? pa_rt_num_cus() : 256;
  size_t blocks = (n + WG - 1) / WG;
  if (blocks > (size_t)8 * cus) blocks = (size_t)8 * cus;
  if (write) PA_LAUNCH(k_pack_set_values<true>, dim3((unsigned)blocks), dim3(WG), 0, cur_stream(), map, pv, meta, packed, n, misses);
  else PA_LAUNCH(k_pack_set_values<false>, dim3((unsigned)blocks), dim3(WG), 0, cur_stream(), map, pv, meta, packed, n, misses);
  return kfail("k_pack_set_values");
}

extern "C" int pa_k_plan_set_values(const unsigned* map, const double* pv, double* val, size_t n) {
  if (n == 0) return 0;
  if (n & 1) { pa_rt_set_error("k_plan_set_values: odd slot count %zu", n); return 1; }
  const size_t npairs = n / 2;
  const int cus = pa_rt_num_cus() > 0 ? pa_rt_num_cus() : 256;
  size_t blocks = (npairs + WG - 1) / WG;
  if (blocks > (size_t)8 * cus) blocks = (size_t)8 * cus;      // eight workgroups per CU, the rest by the stride
  PA_LAUNCH(k_plan_set_values, dim3((unsigned)blocks), dim3(WG), 0, cur_stream(), (const u2v*)map, pv, val, npairs);
  return kfail("k_plan_set_values");
}
