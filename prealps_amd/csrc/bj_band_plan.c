/*
 * bj_band_plan.c -- the dispatch of the band block solve by bandwidth class and panel width (bj_band_plan.h).  The
 * kernels are in bj_band.hip and bj_g4.hip; what is measured about each rule stands next to it here.
 */
#include "bj_band_plan.h"

#include <stdio.h>
#include <string.h>

#include "pa_device.h"      /* pa_bj_wide_window, and bj_g4_plan.h: pa_bj_g4_takes_panel */

int pa_bj_max_R(void) { return PA_BJ_MAX_R; }
int pa_bj_factor_wmax(void) { return PA_BJ_FACTOR_WMAX; }

#define LDS_CU (160 * 1024)      /* bytes of LDS a workgroup may have */
#define REFUSE(...) do { if (why && why_len > 0) snprintf(why, (size_t)why_len, __VA_ARGS__); return 1; } while (0)

/* A wavefront streams its block through two chunk buffers of PA_BJ_BAND_CHUNK records of `rec` doubles, each buffer
 * a multiple of 1 KiB; a workgroup has up to four wavefronts, as many as the LDS holds.  Chunks of 8 steps measured
 * equal or better than 16 and 32 (smaller LDS footprint, more workgroups per CU).  (A ring of three buffers with
 * counted waits measured neutral in round 2 -- 183.6 vs 187.1 us on elasticity, 173.6 vs 172.1 on Poisson, same box:
 * the sweep does not wait for its band -- and its switch is gone; the kernels still take the ring depth as an
 * argument.)  `units` wavefronts of work. */
static int chunked(pa_bj_band_launch_t* L, int rec, int units, char* why, int why_len) {
  L->ch = PA_BJ_BAND_CHUNK;
  L->nbuf = 2;
  L->per_wave = L->nbuf * ((L->ch * rec + 127) & ~127);
  L->waves = LDS_CU / (L->per_wave * 8);
  if (L->waves > 4) L->waves = 4;
  if (L->waves < 1) REFUSE("no room in the LDS: %d bytes per wavefront (at most %d)", L->per_wave * 8, LDS_CU);
  L->lds = L->waves * L->per_wave * 8;
  L->blocks = (units + L->waves - 1) / L->waves;
  L->threads = 64 * L->waves;
  return 0;
}

int pa_bj_band_plan(const pa_bj_band_query_t* q, pa_bj_band_launch_t* L, char* why, int why_len) {
  const int ts = q->ts, wmax = q->wmax;
  memset(L, 0, sizeof(*L));
  if (why && why_len > 0) why[0] = 0;
  /* one copy of the factor on the matrix cores: first wherever the records exist and take the panel.  (k_bj_g4 takes
   * the stride as a number, so it is asked before the strides of the other families are.) */
  if (q->have_g4 && pa_bj_g4_takes_panel(wmax, ts, q->g4_wide)) { L->family = PA_BJ_BAND_G4; return 0; }
  if (ts != 2 && ts != 4 && ts != 8 && ts != 16) REFUSE("unsupported panel stride %d", ts);
  L->ts = L->xs = ts;

  if (q->R < 0) {
    /* wide bands: one workgroup per block, the window of W rows in flight across nw wavefronts of R register sets
     * per lane (1 / 2 / 4 for windows up to 1024 / 2048 / 4096 rows); a lane holds TS columns of each */
    const int R = -q->R, W = pa_bj_wide_window(wmax);
    if (R != 1 && R != 2 && R != 4) REFUSE("a wide class of %d register sets per lane (1, 2 or 4)", R);
    const int nw = (W + 64 * R - 1) / (64 * R);
    if (nw > 16 || ts * R > 16)
      REFUSE("bandwidth %d is too wide for panel stride %d (window %d rows); use more subdomains", wmax, ts, W);
    L->family = PA_BJ_BAND_WIDE;
    L->r = R;
    /* with at most 12 wavefronts (3 per SIMD) a lane has 168 VGPRs and the ring holds twice as many steps */
    L->cap = nw <= 12 ? 768 : 1024;
    L->waves = nw;
    L->blocks = q->count;
    L->threads = 64 * nw;
    return 0;
  }
  if (q->R < 1 || q->R > PA_BJ_MAX_R) REFUSE("bandwidth class R=%d (1 to %d)", q->R, PA_BJ_MAX_R);
  L->r = q->R;

  /* The matrix-core sweep (k_bj_mfma, bands up to 112 in 4 / 6 / 8 tiles of 16 rows: a band and its 16 pivots) costs
   * 210-250 us per apply whatever the panel width (latency: three wavefronts per SIMD, the chain of three lane moves
   * and the pivot tile's MFMA per group of pivots), the register recurrence 172 / 246 / 443 us at 4 / 8 / 16 columns:
   * so it takes the panels of 8 and 16 columns.  PREALPS_BJ_MFMA=0: never; 2: always.  Always four wavefronts: at
   * most 64 KiB, what a launch may have without an attribute. */
  if (wmax <= 112 && ((ts >= 8 && q->mfma == 1) || q->mfma == 2)) {
    L->family = PA_BJ_BAND_MFMA;
    L->tiles = wmax <= 48 ? 4 : wmax <= 80 ? 6 : 8;
    return chunked(L, (wmax + 2) & ~1, q->count, why, why_len);
  }
  /* The register recurrence, one wavefront per block and column group.  (Panels of 8 / 16 columns as 2 / 4 wavefronts
   * of 4 columns each per block measured slower in round 1 -- each wavefront streams the factor again through L2:
   * 257 vs 243 us at 8 columns, 485 vs 434 us at 16 -- and the variant is gone.)
   * Few blocks (a GPU of a multi-GPU run holds 1/8 of them): below one wavefront per SIMD the sweep is latency bound,
   * so a 4-column panel is shared by two wavefronts of 2 columns each (half the FMAs and pivot broadcasts per
   * wavefront; the band is read twice, from L2). */
  if (ts == 4 && q->count < 4 * (q->cus > 0 ? q->cus : 256)) L->ts = 2;
  /* paired records (classes R = 2, 3 at up to 4 columns): two steps per record, wmax + 4 rows of them; else the
   * plain records of wmax + 1 doubles, rounded up to even */
  const int pairs = q->have_pairs && ts <= 4 && (q->R == 2 || q->R == 3);
  L->family = pairs ? PA_BJ_BAND_APPLY_PAIRS : PA_BJ_BAND_APPLY;
  return chunked(L, pairs ? wmax + 4 : (wmax + 2) & ~1, q->count * (L->xs / L->ts), why, why_len);
}
