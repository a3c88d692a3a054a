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

// Does block p = list[blockIdx.x] still repeat its representative rep[p] (bj_share.h) under the new values?  One
// workgroup compares the two assembled bands, nrows (bw + 1) doubles at boff[p] and boff[rep[p]], as 64-bit words
// (the equality of the create: -0.0 is not +0.0), and sets the block's read offsets: the representative's if every
// word is equal, the block's own if not -- the own slot is always written by the set-up kernels that follow.
// cnt[0] += 1 and cnt[1] += (elements of the block's second record) for a block that still shares; the caller zeroes cnt.
// off2 / off2_read are null when no class has second records.
__global__ __launch_bounds__(WG) void k_bj_share_check(const int* __restrict__ list, const int* __restrict__ rep,
                                                      const int* __restrict__ nrows, const int* __restrict__ bw,
                                                      const long long* __restrict__ boff, const double* __restrict__ band,
                                                      const long long* __restrict__ off, const long long* __restrict__ off2,
                                                      long long* __restrict__ off_read, long long* __restrict__ off2_read,
                                                      unsigned long long* __restrict__ cnt) {
  const int p = list[blockIdx.x], r = rep[p];
  const int b = nrows[p], w = bw[p];
  const size_t n = (size_t)b * (size_t)(w + 1);
  const unsigned long long* __restrict__ x = reinterpret_cast<const unsigned long long*>(band + boff[p]);
  const unsigned long long* __restrict__ y = reinterpret_cast<const unsigned long long*>(band + boff[r]);
  int differ = 0;
  for (size_t i = threadIdx.x; i < n; i += WG) differ |= x[i] != y[i];
  differ = __syncthreads_or(differ);
  if (threadIdx.x == 0) {
    const int from = differ ? p : r;
    off_read[p] = off[from];
    if (off2_read) off2_read[p] = off2[from];
    if (!differ) {
      atomicAdd(&cnt[0], 1ull);
      atomicAdd(&cnt[1], (unsigned long long)(8 * ((b + 7) / 8)) * (unsigned long long)(w + 4));
    }
  }
}

}  // namespace

extern "C" int pa_k_bj_share_check(const int* list, int count, const int* rep, const int* nrows, const int* bw,
                                   const long long* boff, const double* band, const long long* off, const long long* off2,
                                   long long* off_read, long long* off2_read, unsigned long long* cnt) {
  if (count <= 0) return 0;
  PA_LAUNCH(k_bj_share_check, dim3((unsigned)count), dim3(WG), 0, cur_stream(), list, rep, nrows, bw, boff, band, off, off2,
            off_read, off2_read, cnt);
  return kfail("k_bj_share_check");
}

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
