// bj_refactor.hip -- assembly of the bands of the block-Jacobi preconditioner on the device, from the panel's
// values and the band map (bj_band_map.h), for the numeric refactorisation in place
// (preAlps_BlockJacobiUpdateValues).  The factorisation and layout kernels that follow are those of the create
// (bj_band.hip, bj_g4.hip), unchanged.
#include "kernels_common.h"

namespace {

// band[boff[blk] + dst[e]] = pv[src[e]] over the chunks of the map; band is zeroed beforehand.  A streaming
// kernel: a workgroup takes a chunk (at most 1024 entries of one block, so the block's base is one scalar load
// per chunk) and the grid strides over the chunks; a lane has four entries in flight.  src and dst are read once,
// coalesced, 4 bytes per lane, hence the nontemporal hint; src ascends inside a block -- the entries are in panel order -- so a wavefront's gather
// from pv touches a few neighbouring cache lines, and pv is the one array read with reuse in L2.  The stores are
// plain vector stores, 8 bytes each, scattered inside one block's band (row-major: a row's entries fall into one
// record of w + 1 doubles); no two entries share a destination, so there is no ordering between them.
__global__ __launch_bounds__(WG) void k_bj_band_assemble(const unsigned* __restrict__ src, const unsigned* __restrict__ dst,
                                                        const int* __restrict__ chunk_blk,
                                                        const unsigned* __restrict__ chunk_first, int nchunks,
                                                        const long long* __restrict__ boff,
                                                        const double* __restrict__ pv, double* __restrict__ band) {
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const unsigned e0 = chunk_first[c], e1 = chunk_first[c + 1];
    double* __restrict__ out = band + boff[chunk_blk[c]];
    for (unsigned base = e0 + threadIdx.x; base < e1; base += 4 * WG) {     // four entries in flight per lane
      unsigned s[4], d[4];
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned e = base + u * WG;
        s[u] = e < e1 ? __builtin_nontemporal_load(src + e) : 0u;
        d[u] = e < e1 ? __builtin_nontemporal_load(dst + e) : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = base + u * WG < e1 ? pv[s[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) if (base + u * WG < e1) out[d[u]] = v[u];
    }
  }
}

}  // namespace

extern "C" int pa_k_bj_band_assemble(const unsigned* src, const unsigned* dst, const int* chunk_blk,
                                     const unsigned* chunk_first, size_t nchunks, const long long* boff,
                                     const double* pv, double* band) {
  if (nchunks == 0) return 0;
  if (nchunks > 0x7fffffffu) { pa_rt_set_error("k_bj_band_assemble: %zu chunks", nchunks); return 1; }
  const int cus = pa_rt_num_cus() > 0 ? pa_rt_num_cus() : 256;
  size_t blocks = nchunks;
  if (blocks > (size_t)8 * cus) blocks = (size_t)8 * cus;      // eight workgroups per CU, the rest by the stride
  PA_LAUNCH(k_bj_band_assemble, dim3((unsigned)blocks), dim3(WG), 0, cur_stream(), src, dst, chunk_blk, chunk_first,
            (int)nchunks, boff, pv, band);
  return kfail("k_bj_band_assemble");
}
