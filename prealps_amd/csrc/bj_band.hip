// bj_band.hip -- the band block solve of the block-Jacobi preconditioner (block_jacobi.c) on CDNA4
// (gfx950): the set-up kernels (band Cholesky of the diagonal blocks, record layout, COO scatter,
// paired records), the apply kernels (k_bj_apply, k_bj_apply_pairs, k_bj_mfma, k_bj_wide), their
// launchers and the dispatch by bandwidth class, pa_k_bj_apply.  The one-copy records of panels of up
// to 4 columns are bj_g4.hip; the dense panel kernels of the ECG iteration are dense_*.hip.
#include "kernels_common.h"

namespace {
// ------------------------------------------------ block-Jacobi setup ----
// Band Cholesky of one diagonal block per workgroup (bands up to PA_BJ_FACTOR_WMAX), right
// looking: the (w+1) x (w+1) window of rows j..j+w lives in LDS (row i in slot i mod (w+1),
// win[slot][d] = A(i, i-d)); step j takes the pivot, scales column j, writes the two sweep
// records the solve kernels read -- forward record j = column j / L(j,j), backward record
// b-1-j = row j / L(j,j) -- and applies the rank-1 update to the rest of the window while
// the next row streams in.  band: the block's rows in factor order, (w+1) doubles each.
__global__ __launch_bounds__(WG) void k_bj_factor(
    const int* __restrict__ list, const int* __restrict__ row0, const int* __restrict__ nrows,
    const int* __restrict__ bw, const long long* __restrict__ off, const long long* __restrict__ boff,
    const double* __restrict__ band, double* __restrict__ Lf, double* __restrict__ Lb,
    double* __restrict__ invd_f, double* __restrict__ invd_b, int* __restrict__ fail) {
  extern __shared__ double win[];
  const int p = list[blockIdx.x];
  const int r0 = row0[p], b = nrows[p], w = bw[p];
  const int ld = w + 1, wr = (w + 2) & ~1;
  const double* __restrict__ A = band + boff[p];
  double* __restrict__ f = Lf + off[p];
  double* __restrict__ g = Lb + off[p];
  const int tid = threadIdx.x;
  const int nfirst = (b < ld ? b : ld) * ld;
  for (int e = tid; e < nfirst; e += WG) win[e] = A[e];
  __syncthreads();
  for (int j = 0; j < b; ++j) {
    const int rj = j % ld, jb = b - 1 - j;
    const double d0 = win[rj * ld];
    if (!(d0 > 0.0) && tid == 0) atomicCAS(fail, 0, r0 + j + 1);
    const double piv = (d0 > 0.0) ? sqrt(d0) : __longlong_as_double(0x7ff8000000000000LL);
    const double invp = 1.0 / piv;
    for (int t = tid; t < w; t += WG) {
      const int dd = t + 1, i = j + dd;
      g[(size_t)jb * wr + t] = (j - dd >= 0) ? win[rj * ld + dd] * invp : 0.0;
      if (i < b) {
        const int ri = i % ld;
        const double l = win[ri * ld + dd] / piv;
        win[ri * ld + dd] = l;
        f[(size_t)j * wr + t] = l * invp;
      }
    }
    if (tid == 0) { invd_f[r0 + j] = invp; invd_b[r0 + jb] = invp; }
    __syncthreads();
    const int nb = (b - 1 - j) < w ? (b - 1 - j) : w;     // rows below the pivot inside the band
    for (int e = tid; e < nb * nb; e += WG) {
      const int a = e / nb + 1, c = e - (a - 1) * nb + 1;
      if (c <= a) {
        const int ri = (j + a) % ld, rk = (j + c) % ld;
        win[ri * ld + (a - c)] -= win[ri * ld + a] * win[rk * ld + c];
      }
    }
    const int in = j + w + 1;                             // the row that takes over slot rj
    if (in < b)
      for (int e = tid; e < ld; e += WG) win[rj * ld + e] = A[(size_t)in * ld + e];
    __syncthreads();
  }
}

// The same factorisation for wider bands (up to 4032), blocked by NB columns, one workgroup of
// 1024 threads per block.  The band is stored diagonal-major (A(i, i-d) at band[d*b + i]) so
// that a wavefront working on one diagonal touches consecutive addresses.  Per block column:
// the NB x NB diagonal block is factored by one thread in LDS; one thread per row solves the
// panel rows against it and leaves them in LDS (w x NB doubles: NB = 16 / 8 / 4 for bands up
// to 1024 / 2048 / 4096); then the trailing window is updated diagonal by diagonal, the
// diagonals dealt out to the wavefronts: A(i, i-d) -= panel[i] . panel[i-d].
template <int NB>
__global__ __launch_bounds__(1024) void k_bj_factor_big(
    const int* __restrict__ list, const int* __restrict__ row0, const int* __restrict__ nrows,
    const int* __restrict__ bw, const long long* __restrict__ boff, double* __restrict__ band,
    int* __restrict__ fail) {
  extern __shared__ double sm[];
  const int p = list[blockIdx.x];
  const int b = nrows[p], w = bw[p];
  double* __restrict__ A = band + boff[p];
  double* panel = sm;                        // [row][NB]
  double* D = sm + (size_t)w * NB;           // [NB][NB], lower triangle of the diagonal block
  const int tid = threadIdx.x, nt = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nw = nt >> 6;
  for (int J = 0; J < b; J += NB) {
    const int nbk = (b - J) < NB ? (b - J) : NB;
    for (int e = tid; e < NB * NB; e += nt) {
      const int r = e / NB, c = e % NB;
      D[e] = (r < nbk && c <= r) ? A[(size_t)(r - c) * b + J + r] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    if (tid == 0) {
      for (int c = 0; c < nbk; ++c) {
        double d = D[c * NB + c];
        for (int k = 0; k < c; ++k) d -= D[c * NB + k] * D[c * NB + k];
        if (!(d > 0.0)) { atomicCAS(fail, 0, row0[p] + J + c + 1); d = __longlong_as_double(0x7ff8000000000000LL); }
        const double piv = sqrt(d);
        D[c * NB + c] = piv;
        for (int r = c + 1; r < nbk; ++r) {
          double v = D[r * NB + c];
          for (int k = 0; k < c; ++k) v -= D[r * NB + k] * D[c * NB + k];
          D[r * NB + c] = v / piv;
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < nbk * NB; e += nt) {
      const int r = e / NB, c = e % NB;
      if (c <= r) A[(size_t)(r - c) * b + J + r] = D[e];
    }
    // panel: rows below the diagonal block that reach into these columns
    const int i0 = J + nbk;
    const int last = (J + nbk + w) < b ? (J + nbk + w) : b;
    const int np_ = last - i0;
    for (int ip = tid; ip < np_; ip += nt) {
      const int i = i0 + ip;
      double x[NB];
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const int dd = i - (J + c);
        x[c] = (c < nbk && dd <= w) ? A[(size_t)dd * b + i] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        if (c < nbk) {
          double v = x[c];
#pragma unroll
          for (int k = 0; k < c; ++k) v -= x[k] * D[c * NB + k];
          x[c] = v / D[c * NB + c];
        }
      }
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const int dd = i - (J + c);
        panel[(size_t)ip * NB + c] = x[c];
        if (c < nbk && dd <= w) A[(size_t)dd * b + i] = x[c];
      }
    }
    __syncthreads();
    // trailing update of the window, diagonal by diagonal
    for (int ipb = 0; ipb < np_; ipb += 64) {
      const int ip = ipb + lane;
      const bool valid = ip < np_;
      double pr[NB];
#pragma unroll
      for (int c = 0; c < NB; ++c) pr[c] = valid ? panel[(size_t)ip * NB + c] : 0.0;
      const int dtop = (ipb + 63) < w ? (ipb + 63) : w;
      for (int d = wave; d <= dtop; d += nw) {
        if (valid && d <= ip) {
          const double* q = panel + (size_t)(ip - d) * NB;
          double sum = 0.0;
#pragma unroll
          for (int c = 0; c < NB; ++c) sum = fma(pr[c], q[c], sum);
          A[(size_t)d * b + i0 + ip] -= sum;
        }
      }
    }
    __syncthreads();
  }
}

// band[off[e]] = val[e]: assembly of the wide bands from the block's lower-triangle entries
// (shipping the mostly empty band itself would cost gigabytes over PCIe)
__global__ __launch_bounds__(WG) void k_scatter(size_t n, const long long* __restrict__ off,
                                               const double* __restrict__ val, double* __restrict__ dst) {
  const size_t stride = (size_t)gridDim.x * WG;
  for (size_t e = (size_t)blockIdx.x * WG + threadIdx.x; e < n; e += stride) dst[off[e]] = val[e];
}

// Sweep records and 1/L(j,j) from a factored diagonal-major band: forward record j = column j
// of L over L(j,j), backward record j = row b-1-j over its diagonal; `wide` records are in
// window-slot order (k_bj_wide), the others [d = 1..w | 0] (k_bj_apply).
__global__ __launch_bounds__(WG) void k_bj_layout_big(
    const int* __restrict__ list, const int* __restrict__ row0, const int* __restrict__ nrows,
    const int* __restrict__ bw, const long long* __restrict__ off, const long long* __restrict__ boff,
    const double* __restrict__ band, int wide_from, double* __restrict__ Lf, double* __restrict__ Lb,
    double* __restrict__ invd_f, double* __restrict__ invd_b) {
  const int p = list[blockIdx.y];
  const int b = nrows[p], w = bw[p], r0 = row0[p];
  const double* __restrict__ A = band + boff[p];
  const bool wide = w > wide_from;
  const size_t reclen = wide ? (size_t)pa_bj_wide_window(w) : (size_t)((w + 2) & ~1);
  double* __restrict__ f = Lf + off[p];
  double* __restrict__ g = Lb + off[p];
  for (int j = blockIdx.x; j < b; j += gridDim.x) {
    const int jr = b - 1 - j;
    const double idf = 1.0 / A[j], idb = 1.0 / A[jr];
    if (threadIdx.x == 0) { invd_f[r0 + j] = idf; invd_b[r0 + j] = idb; }
    for (int dd = 1 + threadIdx.x; dd <= w; dd += WG) {
      const size_t slot = wide ? (size_t)(j + dd) % reclen : (size_t)(dd - 1);
      if (j + dd < b) f[(size_t)j * reclen + slot] = A[(size_t)dd * b + j + dd] * idf;
      if (jr - dd >= 0) g[(size_t)j * reclen + slot] = A[(size_t)dd * b + jr] * idb;
    }
  }
}

// -------------------------------------------------------- block-Jacobi ----
// Exact solve with one SPD diagonal block per wavefront: banded Cholesky
// factor (RCM order, factored at setup) applied as two systolic sweeps.  The
// W = 64*R rows in flight live in registers, row (j mod W) in lane (j mod 64)
// of register set (j/64 mod R); at step j the pivot y_j is broadcast with
// v_readlane and every lane updates the rows j+1..j+w it holds.
//
// The band is the only large operand and it is read exactly once per sweep:
// step j needs the record [L(j+1..j+w, j) / L(j,j) | 0] (wr doubles).
// Records are streamed HBM -> LDS in chunks of CH steps with LDS-DMA
// (global_load_lds_dwordx4: 1 KiB per wave instruction, no VGPRs), double
// buffered per wave so chunk c+1 is in flight while chunk c is consumed.
typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef const __attribute__((address_space(1))) void* glb_void_ptr;

template <int CH>
__device__ __forceinline__ void bj_issue_chunk(const double* __restrict__ rec, int wr, int chunk,
                                               double* lbuf, int lane) {
  const int nbytes = CH * wr * 8;
  const char* g = reinterpret_cast<const char*>(rec) + (size_t)chunk * nbytes + lane * 16;
  char* l = reinterpret_cast<char*>(lbuf);
  for (int o = 0; o < nbytes; o += 1024)
    __builtin_amdgcn_global_load_lds((glb_void_ptr)(g + o), (lds_void_ptr)(l + o), 16, 0, 0);
}

// Record of step j (wr = w + 1 rounded up to even, doubles):
//   r[d-1] = L(j+d, j) / L(j, j), d = 1..w      r[w] = 0
// The band is pre-divided by its pivot, so a step is a_i -= (L_ij / L_jj) a_j
// with a_j read straight from its lane (no multiply on the critical path);
// y_j = a_j / L_jj is formed once per row when its block of 64 is stored.
// A lane that holds row j+d reads r[min(d-1, w)] (d-1 taken as unsigned): rows
// outside the band, the pivot row itself (d = 0) and rows already solved
// (d < 0) all land on the zero, so the update needs no branch.  A solved row is
// never touched again, so the block's 64 results stay in their lanes and are
// scaled and stored together when the block is done.
template <int R>
struct bj_vals {
  double lv[R];
};

template <int R, int K>
__device__ __forceinline__ void bj_load_step(const double* __restrict__ r, int l, int w, int lane,
                                             bj_vals<R>& v) {
#pragma unroll
  for (int k2 = 0; k2 < R; ++k2) {
    const int rel = (k2 - K + R) % R;
    v.lv[k2] = 0.0;
    if (rel == 0 || l >= rel * 64 - w) {       // wave-uniform: does set k2 touch the band at all?
      const unsigned d1 = (unsigned)(rel * 64 + lane - l - 1);
      const unsigned idx = min(d1, (unsigned)w);
      v.lv[k2] = r[idx];
    }
  }
}

// A full chunk of CH steps with the first NA register sets (counted from the pivots' own set)
// inside the band: straight-line code, the band values of four steps at a time read from LDS
// up front, no branch and no scalar bookkeeping per step.  (Sets beyond NA would only meet the zero slot.)
template <int TS, int R, int CH, int K, int NA>
__device__ __forceinline__ void bj_chunk_fast(double (&acc)[R][TS], const double* cur, int lc, int w,
                                              int wr, int lane) {
  constexpr int G = 4;                              // steps whose band values are in registers at once
#pragma unroll
  for (int s0 = 0; s0 < CH; s0 += G) {
    double cf[G][NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int a0 = a * 64 + lane - lc - s0 - 1;   // d - 1 of step s0 for this set
#pragma unroll
      for (int s = 0; s < G; ++s) {
        const unsigned idx = min((unsigned)(a0 - s), (unsigned)w);
        cf[s][a] = cur[(s0 + s) * wr + idx];
      }
    }
#pragma unroll
    for (int s = 0; s < G; ++s) {
      double y[TS];
#pragma unroll
      for (int c = 0; c < TS; ++c) y[c] = readlane_f64(acc[K][c], lc + s0 + s);
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int k2 = (K + a) % R;
#pragma unroll
        for (int c = 0; c < TS; ++c) acc[k2][c] = fma(-cf[s][a], y[c], acc[k2][c]);
      }
    }
  }
}

// The same chunk from PAIRED records (k_bj_pairs): a chunk is two sub-blocks of four steps, a
// sub-block holds, for each of its two pivot pairs, one double2 per target row rho = row - first
// pivot of the sub-block (0 .. w + 3; row 0 is all zero and doubles as the slot of every row outside
// the band): the band values a lane needs for four steps are two ds_read_b128 at one index instead
// of four ds_read_b64 at four clamped indices.
template <int TS, int R, int CH, int K, int NA>
__device__ __forceinline__ void bj_chunk_pairs(double (&acc)[R][TS], const double* cur, int lc, int w, int lane) {
  const int nr = w + 4;
#pragma unroll
  for (int sb = 0; sb < CH / 4; ++sb) {
    const double2* blk = reinterpret_cast<const double2*>(cur + (size_t)sb * 4 * nr);
    double2 cf[NA][2];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const unsigned rho = (unsigned)(a * 64 + lane - lc - 4 * sb);
      const unsigned idx = rho < (unsigned)nr ? rho : 0u;
      cf[a][0] = blk[idx];
      cf[a][1] = blk[nr + idx];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double y[TS];
#pragma unroll
      for (int c = 0; c < TS; ++c) y[c] = readlane_f64(acc[K][c], lc + 4 * sb + s);
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int k2 = (K + a) % R;
        const double v = (s & 1) ? cf[a][s >> 1].y : cf[a][s >> 1].x;
#pragma unroll
        for (int c = 0; c < TS; ++c) acc[k2][c] = fma(-v, y[c], acc[k2][c]);
      }
    }
  }
}

// The chunks of a sweep go through a ring of `nbuf` LDS buffers (`lstride` doubles apart).  Two
// buffers: chunk c+1 is in flight while chunk c is consumed, and c has landed once every
// outstanding VMEM operation of the wave is done.  Three buffers (narrow bands): c+1 AND c+2 are in
// flight -- at 5 TB/s the loaded memory latency is longer than the 8 steps a chunk lasts, so one
// chunk of look-ahead left the wave waiting -- and c has landed once at most the `nld` load
// instructions of chunk c+1 are outstanding (loads return in order; younger ones only make the
// wait stricter).
__device__ __forceinline__ void bj_wait_chunk(int nld_allowed) {
  switch (nld_allowed) {
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

template <int TS, int R, int CH, int K, int LAY = 0>
__device__ __forceinline__ void bj_block(double (&acc)[R][TS], int lim, int& chunk, int b, int w, int wr,
                                         const double* __restrict__ rec, double* lds0, int lstride, int nbuf,
                                         int nld, int lane) {
  for (int lc = 0; lc < lim; lc += CH, ++chunk) {
    bj_wait_chunk((nbuf == 3 && (chunk + 1) * CH < b) ? nld : 0);
    const double* cur = lds0 + (size_t)(chunk % nbuf) * lstride;
    {
      const int ahead = chunk + nbuf - 1;
      if (ahead * CH < b) bj_issue_chunk<CH>(rec, wr, ahead, lds0 + (size_t)(ahead % nbuf) * lstride, lane);
    }
    if constexpr (LAY == 1) {            // paired records: every chunk is whole (zero padded)
      const int lmax = lc + CH - 1;
      if (R >= 3 && lmax >= 128 - w) bj_chunk_pairs<TS, R, CH, K, (R >= 3 ? 3 : 1)>(acc, cur, lc, w, lane);
      else if (R >= 2 && lmax >= 64 - w) bj_chunk_pairs<TS, R, CH, K, (R >= 2 ? 2 : 1)>(acc, cur, lc, w, lane);
      else bj_chunk_pairs<TS, R, CH, K, 1>(acc, cur, lc, w, lane);
      continue;
    }
    const int send = (lim - lc) < CH ? (lim - lc) : CH;
    if constexpr (R <= 3 && TS <= 4) {   // (no gain measured at 8 columns; 16 would spill)
      if (send == CH) {
        // sets the last step of the chunk reaches (wave-uniform): rel is inside the band from
        // step l >= rel*64 - w on
        const int lmax = lc + CH - 1;
        if (R >= 3 && lmax >= 128 - w) bj_chunk_fast<TS, R, CH, K, (R >= 3 ? 3 : 1)>(acc, cur, lc, w, wr, lane);
        else if (R >= 2 && lmax >= 64 - w) bj_chunk_fast<TS, R, CH, K, (R >= 2 ? 2 : 1)>(acc, cur, lc, w, wr, lane);
        else bj_chunk_fast<TS, R, CH, K, 1>(acc, cur, lc, w, wr, lane);
        continue;
      }
    }
    bj_vals<R> nv;
    bj_load_step<R, K>(cur, lc, w, lane, nv);
    for (int s = 0; s < send; ++s) {
      const int l = lc + s;
      const bj_vals<R> cv = nv;
      if (s + 1 < send) bj_load_step<R, K>(cur + (s + 1) * wr, l + 1, w, lane, nv);
      double y[TS];
#pragma unroll
      for (int c = 0; c < TS; ++c) y[c] = readlane_f64(acc[K][c], l);
#pragma unroll
      for (int k2 = 0; k2 < R; ++k2) {
        const int rel = (k2 - K + R) % R;
        if (rel == 0 || l >= rel * 64 - w) {
#pragma unroll
          for (int c = 0; c < TS; ++c) acc[k2][c] = fma(-cv.lv[k2], y[c], acc[k2][c]);
        }
      }
    }
  }
}

template <int TS, int R, int CH, int K, int XS, int LAY = 0>
__device__ __forceinline__ void bj_blocks(double (&acc)[R][TS], int (&rowid)[R], int jb, int& chunk, int b,
                                          int w, int wr, const double* __restrict__ rec,
                                          const double* __restrict__ invd,
                                          const int* __restrict__ iomap, size_t rowbase,
                                          const double* __restrict__ src, double* __restrict__ dst,
                                          double* lds0, int lstride, int nbuf, int nld, int lane) {
  if constexpr (K < R) {
    constexpr int W = 64 * R;
    const int j0 = jb + K * 64;
    if (j0 < b) {
      double nxt[TS];
      double idl = 0.0;
      int nrow = 0;
      const int jn = j0 + W + lane;
      if (j0 + lane < b) idl = invd[j0 + lane];
      if (jn < b) { nrow = iomap[jn]; load_row_s<TS, XS>(src, rowbase + nrow, nxt); }
      else
#pragma unroll
        for (int c = 0; c < TS; ++c) nxt[c] = 0.0;
      const int lim = (b - j0) < 64 ? (b - j0) : 64;
      bj_block<TS, R, CH, K, LAY>(acc, lim, chunk, b, w, wr, rec, lds0, lstride, nbuf, nld, lane);
      if (lane < lim) {
        double y[TS];
#pragma unroll
        for (int c = 0; c < TS; ++c) y[c] = acc[K][c] * idl;
        store_row_s<TS, XS>(dst, rowbase + rowid[K], y);
      }
#pragma unroll
      for (int c = 0; c < TS; ++c) acc[K][c] = nxt[c];
      rowid[K] = nrow;
    }
    bj_blocks<TS, R, CH, K + 1, XS, LAY>(acc, rowid, jb, chunk, b, w, wr, rec, invd, iomap, rowbase, src, dst, lds0,
                                lstride, nbuf, nld, lane);
  }
}

template <int TS, int R, int CH, int XS, int LAY = 0>
__device__ __forceinline__ void bj_sweep(int b, int w, int wr, const double* __restrict__ rec,
                                         const double* __restrict__ invd,
                                         const int* __restrict__ iomap, size_t rowbase,
                                         const double* __restrict__ src, double* __restrict__ dst,
                                         double* lds0, int lstride, int nbuf, int nld, int lane) {
  constexpr int W = 64 * R;
  double acc[R][TS];
  int rowid[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int j = k * 64 + lane;
    rowid[k] = 0;
    if (j < b) { rowid[k] = iomap[j]; load_row_s<TS, XS>(src, rowbase + rowid[k], acc[k]); }
    else
#pragma unroll
      for (int c = 0; c < TS; ++c) acc[k][c] = 0.0;
  }
  bj_issue_chunk<CH>(rec, wr, 0, lds0, lane);
  if (nbuf == 3 && CH < b) bj_issue_chunk<CH>(rec, wr, 1, lds0 + lstride, lane);
  int chunk = 0;
  for (int jb = 0; jb < b; jb += W)
    bj_blocks<TS, R, CH, 0, XS, LAY>(acc, rowid, jb, chunk, b, w, wr, rec, invd, iomap, rowbase, src, dst, lds0, lstride,
                            nbuf, nld, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// XS = panel stride: XS = TS, or a multiple of it when the panel is split by columns among XS/TS
// wavefronts (opt-in, see bj_launch).
// OCC = wavefronts per SIMD the register allocation must leave room for (1: no constraint).  All
// blocks of a class take equally long, so what counts is whether they fit the chip in ONE round:
// 5670 blocks on 1024 SIMDs need 6 resident wavefronts per SIMD (4 meant a second, nearly empty
// round behind the first).
template <int TS, int R, int CH, int XS, int OCC>
__global__ __launch_bounds__(256, OCC) void k_bj_apply(
    const int* __restrict__ list, int count, const int* __restrict__ row0,
    const int* __restrict__ nrows, const int* __restrict__ bw, const long long* __restrict__ off,
    const int* __restrict__ map_f, const int* __restrict__ map_b, const double* __restrict__ Lf,
    const double* __restrict__ Lb, const double* __restrict__ invd_f,
    const double* __restrict__ invd_b, int lds_per_wave, int nbuf, const double* __restrict__ in,
    double* __restrict__ out) {
  extern __shared__ double smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  constexpr int NS = XS / TS;
  const int unit = blockIdx.x * (blockDim.x >> 6) + wave;
  const int pi = unit / NS;
  if (pi >= count) return;
  const int coff = (unit % NS) * TS;
  // everything that steers the sweep is wave-uniform: keep it in SGPRs
  const int p = __builtin_amdgcn_readfirstlane(list[pi]);
  const int r0 = __builtin_amdgcn_readfirstlane(row0[p]);
  const int b = __builtin_amdgcn_readfirstlane(nrows[p]);
  const int w = __builtin_amdgcn_readfirstlane(bw[p]);
  const int wr = (w + 2) & ~1;
  const long long o64 = off[p];
  const size_t o = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(o64 >> 32)) << 32) |
                   (unsigned)__builtin_amdgcn_readfirstlane((int)o64);
  double* lds0 = smem + (size_t)wave * lds_per_wave;
  const int lstride = lds_per_wave / nbuf;
  const int nld = (CH * wr * 8 + 1023) >> 10;      // load instructions per chunk of THIS block
  const int nb = nld <= 4 ? nbuf : 2;               // (the counted wait knows 1..4)
  // forward: L y = x (y goes to `out`), backward: L^T z = y in place
  bj_sweep<TS, R, CH, XS>(b, w, wr, Lf + o, invd_f + r0, map_f + r0, (size_t)r0, in + coff, out + coff, lds0, lstride, nb, nld, lane);
  __threadfence_block();
  bj_sweep<TS, R, CH, XS>(b, w, wr, Lb + o, invd_b + r0, map_b + r0, (size_t)r0, out + coff, out + coff, lds0, lstride, nb, nld, lane);
}

// k_bj_apply on paired records (bj_chunk_pairs): Lf2 / Lb2 at off2[p], 8 (w + 4) doubles per chunk.
template <int TS, int R, int CH, int XS>
__global__ __launch_bounds__(256) void k_bj_apply_pairs(
    const int* __restrict__ list, int count, const int* __restrict__ row0,
    const int* __restrict__ nrows, const int* __restrict__ bw, const long long* __restrict__ off2,
    const int* __restrict__ map_f, const int* __restrict__ map_b, const double* __restrict__ Lf2,
    const double* __restrict__ Lb2, const double* __restrict__ invd_f,
    const double* __restrict__ invd_b, int lds_per_wave, int nbuf, const double* __restrict__ in,
    double* __restrict__ out) {
  extern __shared__ double smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  constexpr int NS = XS / TS;
  const int unit = blockIdx.x * (blockDim.x >> 6) + wave;
  const int pi = unit / NS;
  if (pi >= count) return;
  const int coff = (unit % NS) * TS;
  const int p = __builtin_amdgcn_readfirstlane(list[pi]);
  const int r0 = __builtin_amdgcn_readfirstlane(row0[p]);
  const int b = __builtin_amdgcn_readfirstlane(nrows[p]);
  const int w = __builtin_amdgcn_readfirstlane(bw[p]);
  const int wr2 = w + 4;
  const int nld = (CH * wr2 * 8 + 1023) >> 10;
  const int nb = nld <= 4 ? nbuf : 2;
  const long long o64 = off2[p];
  const size_t o = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(o64 >> 32)) << 32) |
                   (unsigned)__builtin_amdgcn_readfirstlane((int)o64);
  double* lds0 = smem + (size_t)wave * lds_per_wave;
  const int lstride = lds_per_wave / nbuf;
  bj_sweep<TS, R, CH, XS, 1>(b, w, wr2, Lf2 + o, invd_f + r0, map_f + r0, (size_t)r0, in + coff, out + coff, lds0, lstride, nb, nld, lane);
  __threadfence_block();
  bj_sweep<TS, R, CH, XS, 1>(b, w, wr2, Lb2 + o, invd_b + r0, map_b + r0, (size_t)r0, out + coff, out + coff, lds0, lstride, nb, nld, lane);
}

// Paired records from the plain ones: sub-block q = steps 4q .. 4q + 3; entry (pair, rho) =
// the two pivots' coefficients for row 4q + rho (zero outside the band and past the last step).
__global__ __launch_bounds__(WG) void k_bj_pairs(const int* __restrict__ list, const int* __restrict__ nrows,
                                                 const int* __restrict__ bw, const long long* __restrict__ off,
                                                 const long long* __restrict__ off2, const double* __restrict__ L,
                                                 double* __restrict__ L2) {
  const int p = list[blockIdx.x];
  const int b = nrows[p], w = bw[p], wr = (w + 2) & ~1, nr = w + 4;
  const double* __restrict__ rec = L + off[p];
  double2* __restrict__ dst = reinterpret_cast<double2*>(L2 + off2[p]);
  const int nsub = 2 * ((b + 7) / 8);
  const int total = nsub * 2 * nr;
  for (int e = threadIdx.x; e < total; e += WG) {
    const int q = e / (2 * nr), r = e - q * 2 * nr, pr = r / nr, rho = r - pr * nr;
    double v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int l = 4 * q + 2 * pr + h, d = rho - (2 * pr + h);      // pivot, distance row - pivot
      v[h] = (l < b && d >= 1 && d <= w) ? rec[(size_t)l * wr + d - 1] : 0.0;
    }
    dst[e] = make_double2(v[0], v[1]);
  }
}

// Wide bands (RCM bandwidth > 448: few, large subdomains).  One workgroup of up to 16
// wavefronts per subdomain; the W = 64*R*NW rows in flight are spread over the waves'
// registers exactly as in the one-wave kernel.  Per step the owning wave broadcasts the
// pivot through LDS (double buffered, one raw s_barrier per step), then every wave updates
// its rows.  Records are stored in window-slot order -- the value for target row i sits at
// column i mod W -- so a lane reads the same column of every record: no index arithmetic,
// coalesced, and prefetched D steps ahead in registers.
// ---- the same sweeps on the f64 matrix cores (panels of 8 / 16 columns) ----
// The window is kept as NT tiles of 16 rows in the C/D layout of v_mfma_f64_16x16x4 (lane l,
// register r <-> tile row (l>>4) + 4r, panel column l&15).  Four pivots at a time: they are
// the four rows of one register of the pivot tile, so once they are settled among themselves
// (three ds_bpermute steps) that register *is* the B operand
// Y[k = l>>4][j = l&15] of the rank-4 update  tile -= L[rows of tile][4 pivots] * Y  -- no
// data movement.  The A operand is the band value of (row l&15 of the tile, pivot l>>4), one
// LDS read per lane and tile.  Per step this costs a quarter of the v_readlane / v_fma_f64
// recurrence above at 16 columns.  Same records, same LDS-DMA chunks of 8 steps.
template <int TS, int NT, int TP>
__device__ __forceinline__ void bjm_tile(mfma_d4 (&acc)[NT], int (&rid)[NT][4], int g, int& chunk, int b,
                                         int w, int wr, const double* __restrict__ rec,
                                         const double* __restrict__ invd, const int* __restrict__ iomap,
                                         size_t rowbase, const double* __restrict__ src,
                                         double* __restrict__ dst, double* lds0, double* lds1, int lane) {
  const int lo = lane & 15, hi = lane >> 4;
  const double* cur = lds0;
  // what the hand-over at the end needs -- 1/L(j,j) of the tile's rows, the ids of the rows
  // that take over the slot, then their values -- is fetched right *behind* the two chunk
  // waits, so that every s_waitcnt vmcnt(0) only meets loads issued eight steps earlier
  double idl[4], nxt[4];
  int nid[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { idl[r] = 0.0; nid[r] = 0; nxt[r] = 0.0; }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if ((r & 1) == 0) {   // a new chunk of 8 steps starts with this group of four pivots
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      cur = (chunk & 1) ? lds1 : lds0;
      if ((chunk + 1) * 8 < b) bj_issue_chunk<8>(rec, wr, chunk + 1, (chunk & 1) ? lds0 : lds1, lane);
      ++chunk;
      if (r == 0) {
#pragma unroll
        for (int r2 = 0; r2 < 4; ++r2) {   // branch-free: past the end, entry 0 (masked when used)
          const int j = 16 * g + hi + 4 * r2, jn = j + 16 * NT;
          idl[r2] = invd[j < b ? j : 0];
          nid[r2] = iomap[jn < b ? jn : 0];
        }
      } else {              // the ids have landed: the four row loads go out back to back
        const double* sp[4];
#pragma unroll
        for (int r2 = 0; r2 < 4; ++r2) sp[r2] = src + (rowbase + nid[r2]) * TS + (lo < TS ? lo : 0);
#pragma unroll
        for (int r2 = 0; r2 < 4; ++r2) nxt[r2] = *sp[r2];
      }
    }
    const double* grec = cur + (size_t)(4 * (r & 1)) * wr;     // records of this group's pivots
    const double* prec = grec + (size_t)hi * wr;               // record of "my" pivot (k = hi)
    // every band value this group needs, read with explicit ds_read_b64 + one wait: a
    // compiler-visible LDS read of an LDS-DMA target drains all outstanding VMEM first (the
    // chunk in flight), once per read
    double ct[NT], cg[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // pivot a of the group against row hi of the group
      const unsigned ad = (unsigned)(uintptr_t)(lds_void_ptr)(grec + (size_t)a * wr + min(max(hi - a - 1, 0), w));
      asm volatile("ds_read_b64 %0, %1" : "=v"(cg[a]) : "v"(ad));
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const unsigned d1 = (unsigned)(16 * t + lo - 4 * r - hi - 1);
      const unsigned ad = (unsigned)(uintptr_t)(lds_void_ptr)(prec + min(d1, (unsigned)w));
      asm volatile("ds_read_b64 %0, %1" : "=v"(ct[t]) : "v"(ad));
    }
    if constexpr (NT == 4)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cg[0]), "+v"(cg[1]), "+v"(cg[2]), "+v"(ct[0]), "+v"(ct[1]), "+v"(ct[2]), "+v"(ct[3]));
    else if constexpr (NT == 6)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cg[0]), "+v"(cg[1]), "+v"(cg[2]), "+v"(ct[0]), "+v"(ct[1]), "+v"(ct[2]), "+v"(ct[3]), "+v"(ct[4]), "+v"(ct[5]));
    else
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cg[0]), "+v"(cg[1]), "+v"(cg[2]), "+v"(ct[0]), "+v"(ct[1]), "+v"(ct[2]), "+v"(ct[3]), "+v"(ct[4]), "+v"(ct[5]), "+v"(ct[6]), "+v"(ct[7]));
    // the four pivots among themselves: the value of pivot a (lanes hi == a) goes down to the
    // rows below it with ds_bpermute -- through the builtin, NOT by hand: `y` is the result of a
    // double-precision matrix instruction (and then of an FMA), which needs wait states before a DS
    // instruction may read it, and the hazard recogniser does not look into inline assembly (bj_g4.hip
    // read stale registers that way; here the nearest producer was 13 instructions ahead: safe by
    // distance only).  The permute touches no LDS memory, so the compiler does not drain the LDS-DMA
    // in flight in front of it (checked in the ISA).  The matrix pipe is the bottleneck of this
    // kernel, so these three steps are not worth four masked MFMAs.
    double y = acc[TP][r];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int from = (a * 16 + lo) * 4;
      const int plo = __builtin_amdgcn_ds_bpermute(from, __double2loint(y));
      const int phi = __builtin_amdgcn_ds_bpermute(from, __double2hiint(y));
      const double ya = __hiloint2double(phi, plo);
      y = fma((hi > a) ? -cg[a] : 0.0, ya, y);
    }
    acc[TP][r] = y;
    // rank-4 update of every tile the band reaches (rows of this group in the pivot tile: done)
    // (tiles past the band meet the record's zero slot: no branch -- a uniform skip makes the
    // compiler merge register states with thousands of moves)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      double cf = ct[t];
      if (t == 0 && (lo >> 2) == r) cf = 0.0;
      acc[(TP + t) % NT] = __builtin_amdgcn_mfma_f64_16x16x4f64(-cf, y, acc[(TP + t) % NT], 0, 0, 0);
    }
  }
  asm volatile("" ::: "memory");   // the next LDS-DMA into these buffers stays behind the reads
  // the tile is solved: scale, store, and take the tile NT further down
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = 16 * g + hi + 4 * r;
    if (j < b && lo < TS) dst[(rowbase + rid[TP][r]) * TS + lo] = acc[TP][r] * idl[r];
    acc[TP][r] = (j + 16 * NT < b && lo < TS) ? nxt[r] : 0.0;
    rid[TP][r] = nid[r];
  }
  __builtin_amdgcn_sched_barrier(0);   // keep the next tile's prefetches from piling up here
}

template <int TS, int NT, int TP>
__device__ __forceinline__ void bjm_tiles(mfma_d4 (&acc)[NT], int (&rid)[NT][4], int g0, int& chunk, int b,
                                          int w, int wr, const double* __restrict__ rec,
                                          const double* __restrict__ invd, const int* __restrict__ iomap,
                                          size_t rowbase, const double* __restrict__ src,
                                          double* __restrict__ dst, double* lds0, double* lds1, int lane) {
  if constexpr (TP < NT) {
    if (16 * (g0 + TP) < b) {
      bjm_tile<TS, NT, TP>(acc, rid, g0 + TP, chunk, b, w, wr, rec, invd, iomap, rowbase, src, dst, lds0, lds1, lane);
      bjm_tiles<TS, NT, TP + 1>(acc, rid, g0, chunk, b, w, wr, rec, invd, iomap, rowbase, src, dst, lds0, lds1, lane);
    }
  }
}

template <int TS, int NT>
__device__ __forceinline__ void bjm_sweep(int b, int w, int wr, const double* __restrict__ rec,
                                          const double* __restrict__ invd, const int* __restrict__ iomap,
                                          size_t rowbase, const double* __restrict__ src,
                                          double* __restrict__ dst, double* lds0, double* lds1, int lane) {
  const int lo = lane & 15, hi = lane >> 4;
  mfma_d4 acc[NT];
  int rid[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 16 * t + hi + 4 * r;
      double v = 0.0;
      int id = 0;
      if (j < b) { id = iomap[j]; if (lo < TS) v = src[(rowbase + id) * TS + lo]; }
      acc[t][r] = v;
      rid[t][r] = id;
    }
  bj_issue_chunk<8>(rec, wr, 0, lds0, lane);
  int chunk = 0;
  for (int g0 = 0; 16 * g0 < b; g0 += NT)
    bjm_tiles<TS, NT, 0>(acc, rid, g0, chunk, b, w, wr, rec, invd, iomap, rowbase, src, dst, lds0, lds1, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int TS, int NT>
__global__ __launch_bounds__(256) void k_bj_mfma(
    const int* __restrict__ list, int count, const int* __restrict__ row0,
    const int* __restrict__ nrows, const int* __restrict__ bw, const long long* __restrict__ off,
    const int* __restrict__ map_f, const int* __restrict__ map_b, const double* __restrict__ Lf,
    const double* __restrict__ Lb, const double* __restrict__ invd_f,
    const double* __restrict__ invd_b, int lds_per_wave, const double* __restrict__ in,
    double* __restrict__ out) {
  extern __shared__ double smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int pi = blockIdx.x * (blockDim.x >> 6) + wave;
  if (pi >= count) return;
  const int p = __builtin_amdgcn_readfirstlane(list[pi]);
  const int r0 = __builtin_amdgcn_readfirstlane(row0[p]);
  const int b = __builtin_amdgcn_readfirstlane(nrows[p]);
  const int w = __builtin_amdgcn_readfirstlane(bw[p]);
  const int wr = (w + 2) & ~1;
  const long long o64 = off[p];
  const size_t o = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(o64 >> 32)) << 32) |
                   (unsigned)__builtin_amdgcn_readfirstlane((int)o64);
  double* lds0 = smem + (size_t)wave * lds_per_wave;
  double* lds1 = lds0 + (lds_per_wave >> 1);
  bjm_sweep<TS, NT>(b, w, wr, Lf + o, invd_f + r0, map_f + r0, (size_t)r0, in, out, lds0, lds1, lane);
  __threadfence_block();
  bjm_sweep<TS, NT>(b, w, wr, Lb + o, invd_b + r0, map_b + r0, (size_t)r0, out, out, lds0, lds1, lane);
}

// The sweep is blocked by 64 pivots.  Phase A: the wave that holds the block's rows
// eliminates them among themselves (in-wave, v_readlane; its 64 x 64 coefficients were
// brought into LDS by LDS-DMA during the previous block) and publishes the 64 solved rows in
// LDS.  Barrier.  Phase B: every wave applies the 64 pivots to its other rows, reading them
// back as LDS broadcasts; the band values come through a register ring that keeps D steps
// (D*R loads per lane, 16-32 KiB per wave) in flight across block boundaries.  Barrier.
// Two barriers per 64 steps instead of one per step; every record entry is read once.
// Always 64 steps: in a short last block the missing pivots are zero rows and their (clamped)
// coefficients multiply zeros, so no step is conditional.  The coefficients arrive in LDS by
// LDS-DMA; they are read with explicit ds_read_b64 + s_waitcnt (8 steps per batch) because a
// compiler-visible LDS read of a DMA target makes the compiler drain every outstanding VMEM
// load of the wave (the whole prefetch ring) first.  `la` = LDS byte address of dl[lane].
template <int TS, int R, int K>
__device__ __forceinline__ void bjb_diag(double (&acc)[R][TS], unsigned la) {
  constexpr int DA = 8;
#pragma unroll
  for (int l0 = 0; l0 < 64; l0 += DA) {
    double q[DA];
#pragma unroll
    for (int u = 0; u < DA; ++u)
      asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(q[u]) : "v"(la), "n"((l0 + u) * 512));
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]));
#pragma unroll
    for (int u = 0; u < DA; ++u) {
      const int l = l0 + u;
#pragma unroll
      for (int c = 0; c < TS; ++c) {
        const double y = readlane_f64(acc[K][c], l);
        acc[K][c] = fma(-q[u], y, acc[K][c]);
      }
    }
  }
  asm volatile("" ::: "memory");   // the next LDS-DMA into this buffer stays behind these reads
}

// 64 records x 64 slots of the diagonal block starting at record `rec0` -> LDS, 1 KiB (two
// records) per instruction; records past the end of the block are clamped (never used).
__device__ __forceinline__ void bjb_issue_diag(const double* __restrict__ rec, int W, int jb, int b,
                                               double* dl, int lane) {
  const int sb = jb % W;
  const int half = lane >> 5, l16 = lane & 31;
  for (int i = 0; i < 32; ++i) {
    int r = jb + 2 * i + half;
    r = r < b ? r : b - 1;
    const char* g = reinterpret_cast<const char*>(rec + (size_t)r * W + sb) + l16 * 16;
    __builtin_amdgcn_global_load_lds((glb_void_ptr)g, (lds_void_ptr)(reinterpret_cast<char*>(dl) + i * 1024), 16, 0, 0);
  }
}

// Phase B of one block; q is the ring (step jb + l sits in q[l % D]), refilled D steps ahead
// (into the next block's records, clamped at the end of the subdomain).  recb = first record
// of the block (wave-uniform, so the loads take a scalar base + the lane's slot offset);
// kskip = the owner's register set, whose slots of these records belong to phase A (-1: none).
template <int TS, int R, int D>
__device__ __forceinline__ void bjb_update(double (&acc)[R][TS], double (&q)[D][R],
                                           const double* __restrict__ recb, int s0, int W, int nleft,
                                           const double (*yb)[TS], int kskip) {
  // the pivots are read P steps ahead of their use (LDS broadcasts, ~100 cycles each)
  constexpr int P = TS * R <= 8 ? 2 : 1;
  double2 yq[P][TS / 2];
#pragma unroll
  for (int a = 0; a < P; ++a)
#pragma unroll
    for (int c = 0; c < TS / 2; ++c) yq[a][c] = reinterpret_cast<const double2*>(yb[a])[c];
#pragma unroll
  for (int l = 0; l < 64; ++l) {
    const int u = l % D;
    double y[TS];
#pragma unroll
    for (int c = 0; c < TS / 2; ++c) { y[2 * c] = yq[l % P][c].x; y[2 * c + 1] = yq[l % P][c].y; }
    if (l + P < 64) {
#pragma unroll
      for (int c = 0; c < TS / 2; ++c) yq[l % P][c] = reinterpret_cast<const double2*>(yb[l + P])[c];
    }
    const int ln = (l + D) < nleft ? (l + D) : nleft - 1;
    const double* __restrict__ pr = recb + (size_t)ln * W;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const double lv = (k == kskip) ? 0.0 : q[u][k];
      q[u][k] = pr[s0 + k * 64];
#pragma unroll
      for (int c = 0; c < TS; ++c) acc[k][c] = fma(-lv, y[c], acc[k][c]);
    }
    // keep the issue order of the source: the scheduler otherwise sinks the LDS reads back
    // next to their uses to save registers and every step eats the full LDS latency
    __builtin_amdgcn_sched_barrier(0);
  }
}

// phase A + hand-over of the owner wave for register set K.  The id of the row that takes
// over the slot was fetched one ownership earlier (rownext), so its load does not hang on a
// fresh index load behind the whole prefetch ring.
template <int TS, int R, int K>
__device__ __forceinline__ void bjb_own(double (&acc)[R][TS], int (&rowid)[R], int (&rownext)[R],
                                        const double* dl, int W, int lim, int jb, int b,
                                        const double* __restrict__ invd, const int* __restrict__ iomap,
                                        size_t rowbase, const double* __restrict__ src,
                                        double* __restrict__ dst, double (*yb)[TS], int lane) {
  double nxt[TS];
  double idl = 0.0;
  const int nrow = rownext[K];
  const int jn = jb + W + lane;
  if (jb + lane < b) idl = invd[jb + lane];
  if (jn < b) load_row<TS>(src, rowbase + nrow, nxt);
  else
#pragma unroll
    for (int c = 0; c < TS; ++c) nxt[c] = 0.0;
  int rn = (jn + W < b) ? iomap[jn + W] : 0;
  bjb_diag<TS, R, K>(acc, (unsigned)(uintptr_t)(lds_void_ptr)(dl + lane));
  // lane l now holds the solved (unscaled) row jb + l: publish, scale, store, take the next row
  double2* yq = reinterpret_cast<double2*>(yb[lane]);
#pragma unroll
  for (int c = 0; c < TS / 2; ++c) yq[c] = make_double2(acc[K][2 * c], acc[K][2 * c + 1]);
  double v[TS];
#pragma unroll
  for (int c = 0; c < TS; ++c) v[c] = acc[K][c] * idl;
  if (lane < lim) store_row<TS>(dst, rowbase + rowid[K], v);
  // the incoming row and the id prefetched for the next ownership are touched here, where
  // their loads have long landed: otherwise the compiler sinks the copy into the loop latch
  // (draining every wave's prefetch ring there) and waits for the id at the start of the next
  // ownership, behind the whole ring
#pragma unroll
  for (int c = 0; c < TS; ++c) { asm volatile("" : "+v"(nxt[c])); acc[K][c] = nxt[c]; }
  rowid[K] = nrow;
  asm volatile("" : "+v"(rn));
  rownext[K] = rn;
}

template <int TS, int R, int D>
__device__ __forceinline__ void bjw_sweep(int b, int W, const double* __restrict__ rec,
                                          const double* __restrict__ invd,
                                          const int* __restrict__ iomap, size_t rowbase,
                                          const double* __restrict__ src, double* __restrict__ dst,
                                          double (*ybuf)[64][TS], double (*dlbuf)[64 * 64], int wave,
                                          int lane, bool active) {
  const int s0 = (active ? wave : 0) * 64 * R + lane;   // slot of register set 0 of this lane
  double acc[R][TS];
  int rowid[R], rownext[R];
  // diagonal coefficients of the first two blocks; later ones are fetched two blocks ahead by
  // the owner that has just finished with the buffer
  if (wave == 0) {
    bjb_issue_diag(rec, W, 0, b, dlbuf[0], lane);
    if (64 < b) bjb_issue_diag(rec, W, 64, b, dlbuf[1], lane);
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int j = s0 + k * 64;
    rowid[k] = 0;
    rownext[k] = (active && j + W < b) ? iomap[j + W] : 0;
    if (active && j < b) { rowid[k] = iomap[j]; load_row<TS>(src, rowbase + rowid[k], acc[k]); }
    else
#pragma unroll
      for (int c = 0; c < TS; ++c) acc[k][c] = 0.0;
  }
  double q[D][R];
#pragma unroll
  for (int u = 0; u < D; ++u)
#pragma unroll
    for (int k = 0; k < R; ++k) q[u][k] = rec[(size_t)(u < b ? u : b - 1) * W + s0 + k * 64];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int jb = 0; jb < b; jb += 64) {
    const int sb = jb % W;
    const int ow = sb / (64 * R), ok = (sb >> 6) % R;   // wave / register set that owns this block
    const bool mine = active && wave == ow;
    const int lim = (b - jb) < 64 ? (b - jb) : 64;
    const int par = (jb >> 6) & 1;
    double (*yb)[TS] = ybuf[par];
    if (mine) {
      double* dl = dlbuf[par];
      if (ok == 0) bjb_own<TS, R, 0>(acc, rowid, rownext, dl, W, lim, jb, b, invd, iomap, rowbase, src, dst, yb, lane);
      if constexpr (R > 1) if (ok == 1) bjb_own<TS, R, 1>(acc, rowid, rownext, dl, W, lim, jb, b, invd, iomap, rowbase, src, dst, yb, lane);
      if constexpr (R > 2) {
        if (ok == 2) bjb_own<TS, R, 2>(acc, rowid, rownext, dl, W, lim, jb, b, invd, iomap, rowbase, src, dst, yb, lane);
        if (ok == 3) bjb_own<TS, R, 3>(acc, rowid, rownext, dl, W, lim, jb, b, invd, iomap, rowbase, src, dst, yb, lane);
      }
    }
    // everything this wave has in flight lands before the barrier (the compiler drains all
    // counters in front of an s_barrier on gfx9 anyway): the published pivots, and the owner's
    // coefficient fetch of the previous block
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // the owner's coefficient buffer is free again: fetch the block after next into it.  The
    // fetch is complete at the next barrier, one block before it is read.
    if (mine && jb + 128 < b) bjb_issue_diag(rec, W, jb + 128, b, dlbuf[par], lane);
    if (active) bjb_update<TS, R, D>(acc, q, rec + (size_t)jb * W, s0, W, b - jb, yb, mine ? ok : -1);
  }
}

// NT = threads the launch may use: with at most 12 wavefronts (3 per SIMD) a lane has 168
// VGPRs and the ring can hold twice as many steps.
template <int TS, int R, int NT>
__global__ __launch_bounds__(NT) void k_bj_wide(
    const int* __restrict__ list, int count, const int* __restrict__ row0,
    const int* __restrict__ nrows, const int* __restrict__ bw, const long long* __restrict__ off,
    const int* __restrict__ map_f, const int* __restrict__ map_b, const double* __restrict__ Lf,
    const double* __restrict__ Lb, const double* __restrict__ invd_f,
    const double* __restrict__ invd_b, const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double ybuf[2][64][TS];
  __shared__ double dl[2][64 * 64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int p = __builtin_amdgcn_readfirstlane(list[blockIdx.x]);
  const int r0 = __builtin_amdgcn_readfirstlane(row0[p]);
  const int b = __builtin_amdgcn_readfirstlane(nrows[p]);
  const int w = __builtin_amdgcn_readfirstlane(bw[p]);
  const int W = pa_bj_wide_window(w);
  const bool active = wave < W / (64 * R);
  const size_t o = (size_t)off[p];
  constexpr int D = (TS == 16 ? 8 : 16) * (NT <= 768 ? 2 : 1) / R;
  bjw_sweep<TS, R, D>(b, W, Lf + o, invd_f + r0, map_f + r0, (size_t)r0, in, out, ybuf, dl, wave, lane, active);
  __threadfence_block();
  __syncthreads();
  bjw_sweep<TS, R, D>(b, W, Lb + o, invd_b + r0, map_b + r0, (size_t)r0, out, out, ybuf, dl, wave, lane, active);
}

}  // namespace

// ---- the launcher of the apply kernels.  Which family serves a class and how it is launched is decided in
// bj_band_plan.c; bj_launch maps that description onto the template instance that has its numbers compiled in.
// One launch of the instance K as L describes it; more than 64 KiB of dynamic LDS needs the attribute, set once per
// instance and size.
template <auto K, typename... A>
static int bj_go(const pa_bj_band_launch_t& L, const char* what, A... args) {
  static int configured = 0;
  if (L.lds > 64 * 1024 && L.lds > configured) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, L.lds);
    if (e != hipSuccess) { pa_rt_set_error("hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e)); return 1; }
    configured = L.lds;
  }
  PA_LAUNCH(K, dim3(L.blocks), dim3(L.threads), (size_t)L.lds, cur_stream(), args...);
  return kfail(what);
}

// what every apply kernel takes first (OFF, LF, LB: the plain or the paired records)
#define BJ_BLOCKS(OFF, LF, LB) list, count, pl->row0, pl->nrows, pl->bw, pl->OFF, pl->map_f, pl->map_b, pl->LF, pl->LB, pl->invd_f, pl->invd_b
// (family, TS, XS -- k_bj_wide: the thread bound / 256 --, R -- k_bj_mfma: the tiles)
#define BJ_KEY(f, a, b, c) ((((f) * 32 + (a)) * 32 + (b)) * 32 + (c))
#define BJ_APPLY(TS, XS, R) case BJ_KEY(PA_BJ_BAND_APPLY, TS, XS, R): \
  return bj_go<&k_bj_apply<TS, R, PA_BJ_BAND_CHUNK, XS, 1>>(L, "k_bj_apply", BJ_BLOCKS(off, Lf, Lb), L.per_wave, L.nbuf, in, out);
#define BJ_APPLY8(TS, XS) BJ_APPLY(TS, XS, 1) BJ_APPLY(TS, XS, 2) BJ_APPLY(TS, XS, 3) BJ_APPLY(TS, XS, 4) BJ_APPLY(TS, XS, 5) BJ_APPLY(TS, XS, 6) BJ_APPLY(TS, XS, 7) BJ_APPLY(TS, XS, 8)
// paired records (pa_k_bj_pairs ran at setup): classes R = 2, 3 at up to 4 columns
#define BJ_PAIRS(TS, XS, R) case BJ_KEY(PA_BJ_BAND_APPLY_PAIRS, TS, XS, R): \
  return bj_go<&k_bj_apply_pairs<TS, R, PA_BJ_BAND_CHUNK, XS>>(L, "k_bj_apply_pairs", BJ_BLOCKS(off2, Lf2, Lb2), L.per_wave, L.nbuf, in, out);
#define BJ_MFMA(TS, NT) case BJ_KEY(PA_BJ_BAND_MFMA, TS, TS, NT): \
  return bj_go<&k_bj_mfma<TS, NT>>(L, "k_bj_mfma", BJ_BLOCKS(off, Lf, Lb), L.per_wave, in, out);
#define BJ_MFMA3(TS) BJ_MFMA(TS, 4) BJ_MFMA(TS, 6) BJ_MFMA(TS, 8)
// one workgroup per block, R register sets per lane: the instance of at most 768 threads and the one of 1024
#define BJ_WIDE(TS, R) \
  case BJ_KEY(PA_BJ_BAND_WIDE, TS, 3, R): return bj_go<&k_bj_wide<TS, R, 768>>(L, "k_bj_wide", BJ_BLOCKS(off, Lf, Lb), in, out); \
  case BJ_KEY(PA_BJ_BAND_WIDE, TS, 4, R): return bj_go<&k_bj_wide<TS, R, 1024>>(L, "k_bj_wide", BJ_BLOCKS(off, Lf, Lb), in, out);

static int bj_launch(const pa_bj_band_launch_t& L, const pa_bj_plan_t* pl, const int* list, int count, const double* in, double* out) {
  switch (BJ_KEY(L.family, L.ts, L.family == PA_BJ_BAND_WIDE ? L.cap >> 8 : L.xs, L.family == PA_BJ_BAND_MFMA ? L.tiles : L.r)) {
    BJ_APPLY8(2, 2) BJ_APPLY8(4, 4) BJ_APPLY8(8, 8) BJ_APPLY8(16, 16) BJ_APPLY8(2, 4)
    BJ_PAIRS(2, 2, 2) BJ_PAIRS(2, 2, 3) BJ_PAIRS(4, 4, 2) BJ_PAIRS(4, 4, 3) BJ_PAIRS(2, 4, 2) BJ_PAIRS(2, 4, 3)
    BJ_MFMA3(2) BJ_MFMA3(4) BJ_MFMA3(8) BJ_MFMA3(16)
    BJ_WIDE(2, 1) BJ_WIDE(2, 2) BJ_WIDE(2, 4) BJ_WIDE(4, 1) BJ_WIDE(4, 2) BJ_WIDE(4, 4) BJ_WIDE(8, 1) BJ_WIDE(8, 2) BJ_WIDE(16, 1)
  }
  pa_rt_set_error("pa_k_bj_apply: no kernel of family %d with TS=%d XS=%d R=%d, %d tiles, %d threads", L.family, L.ts, L.xs, L.r, L.tiles, L.cap);
  return 1;
}

template <int NB>
static int bj_factor_big_launch(const int* list, int count, int wmax, const int* row0, const int* nrows,
                                const int* bw, const long long* boff, double* band, int* fail) {
  const size_t lds = ((size_t)wmax * NB + NB * NB) * 8;
  static size_t configured = 0;
  if (lds > 64 * 1024 && lds > configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bj_factor_big<NB>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return kfail("hipFuncSetAttribute(k_bj_factor_big)");
    configured = lds;
  }
  PA_LAUNCH((k_bj_factor_big<NB>), dim3(count), dim3(1024), lds, cur_stream(), list, row0, nrows, bw,
                     boff, band, fail);
  return kfail("k_bj_factor_big");
}

extern "C" {

int pa_k_bj_factor(const int* list, int count, int wmax, const int* row0, const int* nrows, const int* bw,
                   const long long* off, const long long* boff, const double* band, double* Lf, double* Lb,
                   double* invd_f, double* invd_b, int* fail) {
  if (count <= 0) return 0;
  const size_t lds = (size_t)(wmax + 1) * (wmax + 1) * 8;
  static size_t configured = 0;
  if (lds > 64 * 1024 && lds > configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bj_factor),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return kfail("hipFuncSetAttribute(k_bj_factor)");
    configured = lds;
  }
  PA_LAUNCH(k_bj_factor, dim3(count), dim3(WG), lds, cur_stream(), list, row0, nrows, bw, off, boff,
                     band, Lf, Lb, invd_f, invd_b, fail);
  return kfail("k_bj_factor");
}

int pa_k_scatter(size_t n, const long long* off, const double* val, double* dst) {
  if (n == 0) return 0;
  size_t blocks = (n + WG - 1) / WG;
  if (blocks > 65535) blocks = 65535;
  PA_LAUNCH(k_scatter, dim3((unsigned)blocks), dim3(WG), 0, cur_stream(), n, off, val, dst);
  return kfail("k_scatter");
}

int pa_k_bj_factor_big(const int* list, int count, int wmax, int wide_from, const int* row0, const int* nrows,
                       const int* bw, const long long* off, const long long* boff, double* band, double* Lf, double* Lb,
                       double* invd_f, double* invd_b, int* fail) {
  if (count <= 0) return 0;
  int rc;
  if (wmax <= 1024) rc = bj_factor_big_launch<16>(list, count, wmax, row0, nrows, bw, boff, band, fail);
  else if (wmax <= 2048) rc = bj_factor_big_launch<8>(list, count, wmax, row0, nrows, bw, boff, band, fail);
  else rc = bj_factor_big_launch<4>(list, count, wmax, row0, nrows, bw, boff, band, fail);
  if (rc) return rc;
  PA_LAUNCH(k_bj_layout_big, dim3(512, count), dim3(WG), 0, cur_stream(), list, row0, nrows, bw, off,
                     boff, band, wide_from, Lf, Lb, invd_f, invd_b);
  return kfail("k_bj_layout_big");
}

int pa_k_bj_pairs(const int* list, int count, const int* nrows, const int* bw, const long long* off,
                  const long long* off2, const double* L, double* L2) {
  if (count <= 0) return 0;
  PA_LAUNCH(k_bj_pairs, dim3(count), dim3(WG), 0, cur_stream(), list, nrows, bw, off, off2, L, L2);
  return kfail("k_bj_pairs");
}

/* A Gram block requested from the next block solve in -> out (pa_k_bj_gram_arm), as g_sg for the SpMM */
static struct { const double* in; const double* out; const double* prev; double* partials; int cap, count, armed; } g_bg;

void pa_k_bj_gram_arm(const double* in, const double* out, const double* prev, double* partials, int cap) {
  g_bg.in = in; g_bg.out = out; g_bg.prev = prev; g_bg.partials = partials; g_bg.cap = cap; g_bg.count = 0;
  g_bg.armed = (in && out && prev && partials && cap > 0);
}
static long long g_bg_applies = 0;
long long pa_k_bj_gram_applies(void) { return g_bg_applies; }
void pa_k_bj_gram_disarm(const double* owner) { if (!owner || owner == g_bg.partials) { g_bg.armed = 0; g_bg.count = 0; } }
int pa_k_bj_gram_take(const double* in, const double* out) {
  if (!g_bg.armed || in != g_bg.in || out != g_bg.out) return 0;
  const int n = g_bg.count;
  g_bg.armed = 0; g_bg.count = 0;
  return n;
}

/* Every class of the plan in turn: the query, the plan (bj_band_plan.c; a refusal goes to pa_rt_error() with its
 * reason), the launcher of the family. */
int pa_k_bj_apply(const pa_bj_plan_t* pl, int ts, const double* in, double* out) {
  /* PREALPS_BJ_G4_WIDE=0: 8-column panels stay with k_bj_mfma; PREALPS_BJ_MFMA=0: never k_bj_mfma, 2: at every width */
  static int g4_wide = -1, use_mfma = -1;
  if (g4_wide < 0) {
    const char* e = getenv("PREALPS_BJ_G4_WIDE"); g4_wide = e ? atoi(e) : 1;
    e = getenv("PREALPS_BJ_MFMA"); use_mfma = e ? atoi(e) : 1;
  }
  for (int c = 0; c < pl->nclass; ++c) {
    const int* list = pl->class_list[c];
    const int count = pl->class_count[c];
    if (count <= 0) continue;
    const pa_bj_band_query_t q = {ts, pl->class_R[c], pl->class_wmax[c], count, pl->Lg4 && pl->class_g4[c], pl->Lf2 != nullptr,
                                  g4_wide, use_mfma, pa_rt_num_cus()};
    pa_bj_band_launch_t L;
    char why[160];
    if (pa_bj_band_plan(&q, &L, why, (int)sizeof(why))) { pa_rt_set_error("pa_k_bj_apply: %s", why); return 1; }
    if (L.family != PA_BJ_BAND_G4) {
      if (bj_launch(L, pl, list, count, in, out)) return 1;
      continue;
    }
    /* one copy of the factor, matrix cores (bj_g4.hip) */
    if (ts == 4 && g_bg.armed && pl->nclass == 1 && in == g_bg.in && out == g_bg.out && count <= g_bg.cap) {
      pa_k_bj_g4_gram(g_bg.prev, g_bg.partials);      // this apply also leaves [in | prev]^T out (pa_k_bj_gram_arm)
      g_bg.count = count;
      ++g_bg_applies;
    } else if (g_bg.armed && in == g_bg.in && out == g_bg.out) {
      g_bg.count = 0;
    }
    const int rc = pa_k_bj_g4(pl, list, count, q.wmax, pl->class_bmax[c], ts, ts, in, out, pl->class_ptask ? &pl->class_ptask[c] : nullptr);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
