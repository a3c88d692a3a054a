/*
 * bj_g4_plan.c -- the launch decision of the band block solve (bj_g4_plan.h).  The kernels are in bj_g4.hip; what is
 * measured about each rule stands next to it here.
 */
#include "bj_g4_plan.h"

#include <stdio.h>
#include <string.h>

int pa_bj_g4_max_rows(void) { return PA_BJ_G4_MAX_ROWS; }
int pa_bj_g4_max_band(void) { return PA_BJ_G4_MAX_BAND; }
int pa_bj_g4_max_band8(void) { return PA_BJ_G4_MAX_BAND8; }     /* panels of 5 .. 8 columns (two column sets per wavefront) */

#define LDS_CU (160 * 1024)      /* bytes of LDS a workgroup may have */
#define REFUSE(...) do { if (why && why_len > 0) snprintf(why, (size_t)why_len, __VA_ARGS__); return 1; } while (0)

/* The rule of the PAIR launch: two blocks of one class of identical blocks per wavefront, the
 * record read once for both.  Possible at all: the list has pair tasks with at least one pair, fp64 records, a
 * panel of up to 4 columns, bands the two-set kernels take, and no refresh has split a class since the create (a block
 * that reads its own records again must not be served from its partner's).  PREALPS_BJ_PAIR=1: then always; =0: never;
 * unset: the default below, and then in the many-blocks regime only (at least two blocks per SIMD -- below that the
 * pipelined few-blocks chain stays) and when at least half of the list's blocks have a partner. */
static int pairs(const pa_bj_g4_query_t* q, int simds) {
  if (!q->have_tasks || q->paired < 2 || q->pair_mode == 0 || !q->pair_intact) return 0;
  if (q->bits != 64 || q->xs > 4 || q->ncol > 4 || q->wmax > PA_BJ_G4_MAX_BAND8) return 0;
  if (q->pair_mode == 1) return 1;
  /* measured (profiles/r21_bj_pair_speed.txt): the launch gains where it runs on precomputed operand addresses -- up to
   * 192 rows and bands up to 48 -- and gains nothing or loses elsewhere */
  if (q->bmax > 192 || q->wmax > 48) return 0;
  return q->count >= 2 * simds && 2 * q->paired >= q->count;
}

int pa_bj_g4_plan(const pa_bj_g4_query_t* q, pa_bj_g4_launch_t* L, char* why, int why_len) {
  memset(L, 0, sizeof(*L));
  if (why && why_len > 0) why[0] = 0;
  if (q->bits != 64 && q->bits != 32) REFUSE("records of %d bits (64 or 32)", q->bits);
  if (q->bmax > PA_BJ_G4_MAX_ROWS) REFUSE("blocks of %d rows (at most %d)", q->bmax, PA_BJ_G4_MAX_ROWS);
  if (q->ncol > 8) REFUSE("%d columns (at most 8)", q->ncol);
  const int simds = 4 * (q->cus > 0 ? q->cus : 256);
  const int gram = q->gram && q->xs == 4 && q->ncol == 4;      /* the by-product is an 8 x 4 block of a 4-column panel */

  L->kind = pairs(q, simds) ? PA_BJ_G4_PAIR : PA_BJ_G4_PLAIN;
  L->bits = q->bits;
  L->nt = q->bmax > 224 ? 16 : q->bmax > 192 ? 14 : 12;       /* register tiles of 16 rows */
  L->nc = L->kind == PA_BJ_G4_PAIR || q->ncol > 4 ? 2 : 1;
  /* a record of band w reaches the pivots' tile and (w + 15) / 16 below it */
  L->dq = ((q->wmax + 15) >> 4) + 1;
  if (L->dq < 3) L->dq = 3;
  const int dq_max = L->nc == 1 ? 8 : 6;
  if (L->dq > dq_max)
    REFUSE("a band of %d on %d column set%s (at most %d)", q->wmax, L->nc, L->nc == 1 ? "" : "s", 16 * dq_max - 16);

  if (L->kind == PA_BJ_G4_PAIR) {
    /* ntasks wavefronts of two blocks each.  Always ring 2, the many-blocks configuration the rule picks it for: the
     * hand-kept wait counts of the Gram rows (g4_bwd_chunk: extra) are written for that depth.  A ring buffer is DQ
     * KiB, a compile-time stride (g4_fwd_chunk_q), at most 6: four wavefronts 48 KiB.  Three wavefronts per SIMD by
     * registers (profiles/r21_bj_pair_resources.txt), four by LDS. */
    L->occ = 3;
    L->gp = gram;
    L->ring = 2;
    L->waves = 4;
    L->per_wave = L->ring * L->dq * 128;
    L->blocks = (q->ntasks + L->waves - 1) / L->waves;
    L->last[0] = 2; L->last[1] = 64; L->last[2] = 0; L->last[3] = 1;
  } else {
    /* a chunk is two groups of (wmax + 4) rows x 4 pivots: bits / 8 * (wmax + 4) doubles' worth of bytes */
    const int cbuf = (q->bits / 8 * (q->wmax + 4) + 127) & ~127;      /* doubles per ring buffer, a multiple of 1 KiB */
    const int nld = cbuf >> 7;                                        /* LDS-DMA pieces (1 KiB each) per chunk */
    /* Ring depth.  Many blocks (the chip is filled several wavefronts deep): two buffers, the LDS then allows six
     * wavefronts per SIMD.  Few blocks (fewer than two per SIMD: a shard of a multi-GPU run): a lone wavefront cannot
     * hide the memory latency behind other wavefronts, so up to eight chunks in flight -- as far as the wait counter
     * (15 pieces) and 40 KiB per wavefront allow.  PREALPS_BJ_G4_RING overrides (2, 4, 8).
     * (Fewer resident blocks, so that a block's records survive in the Infinity Cache between its two sweeps, was
     * tried with padded LDS in round 3: 130.4 / 144.9 us against 122.1 us.  The switch is gone.) */
    int ring = q->ring_env == 2 || q->ring_env == 4 || q->ring_env == 8 ? q->ring_env : (q->count < 2 * simds ? 8 : 2);
    while (ring > 2 && ((ring - 1) * nld > 15 || ring * cbuf * 8 > 40 * 1024)) ring >>= 1;
    L->occ = L->nc == 1 ? (L->nt == 12 && L->dq <= 5 ? 5 : 4) : 3;
    L->gp = gram && L->nc == 1;
    L->ring = ring;
    L->per_wave = ring * cbuf;
    L->waves = LDS_CU / (L->per_wave * 8);
    if (L->waves > 4) L->waves = 4;
    if (L->waves < 1) REFUSE("no room in the LDS: %d bytes per wavefront (at most %d)", L->per_wave * 8, LDS_CU);
    /* Few blocks: the software-pipelined group chain with its compile-time ring (PA_BJ_G4_PIPE_RING buffers of DQ KiB
     * and the spare one per wavefront).  fp64 records on one column set of 12 tiles and DQ <= 5 only: everything else
     * takes the plain chain with the deep ring above.  Single-wavefront workgroups: they fill the 160 KiB of a CU to
     * the last buffer set (six blocks per CU at DQ = 5; four-wavefront workgroups of 100 KiB leave room for one).
     * Measured 1 / 2 / 4 wavefronts per workgroup: 20.7 / 24.8 / 20.7 us on 709 blocks (1/8 of the headline problem),
     * 28.5 / 28.3 / 28.9 us on 1418. */
    if (q->bits == 64 && L->nc == 1 && L->nt == 12 && L->dq <= 5 && ring >= 4) {
      L->kind = PA_BJ_G4_PIPE;
      L->occ = 1;
      L->ring = PA_BJ_G4_PIPE_RING;
      L->per_wave = (PA_BJ_G4_PIPE_RING + 1) * L->dq * 128;
      L->waves = 1;
    }
    L->blocks = (q->count + L->waves - 1) / L->waves;
    L->last[0] = L->ring; L->last[1] = q->bits; L->last[2] = L->kind == PA_BJ_G4_PIPE; L->last[3] = 0;
  }
  L->lds = L->waves * L->per_wave * 8;
  return 0;
}
