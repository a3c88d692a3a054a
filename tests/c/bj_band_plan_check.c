/*
 * bj_band_plan_check.c -- runs the dispatch planner of the band block solve (prealps_amd/csrc/bj_band_plan.c:
 * pa_bj_band_plan) on the queries that tests/test_bj_band_plan_cpu.py writes, and dumps the plans for the test to
 * compare.  No judgement here beyond the sanitizers the test builds it with: usage
 * bj_band_plan_check <queries in> <plans out> <reasons out>.
 *
 * Queries file (native binary): records of 9 int32 in the order of pa_bj_band_query_t --
 *   ts R wmax count have_g4 have_pairs g4_wide mfma cus
 * Plans file: one record of 15 int32 per query --
 *   rc why family ts xs r ch tiles cap waves per_wave nbuf lds blocks threads
 * `why` = line (from 0) of the reasons file that holds the text the planner left (an empty line for a plan it made):
 * every distinct text is written once, in the order of its first appearance.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_band_plan.h"

#define WHY_LEN 160
#define WHY_MAX 4096

static char g_why[WHY_MAX][WHY_LEN];
static int g_nwhy;

static int why_id(const char* s) {
  for (int i = 0; i < g_nwhy; ++i)
    if (!strcmp(g_why[i], s)) return i;
  if (g_nwhy == WHY_MAX) { fprintf(stderr, "more than %d distinct reasons\n", WHY_MAX); exit(2); }
  memcpy(g_why[g_nwhy], s, strlen(s) + 1);
  return g_nwhy++;
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s <queries in> <plans out> <reasons out>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  FILE* txt = fopen(argv[3], "w");
  if (!in || !out || !txt) { fprintf(stderr, "cannot open %s / %s / %s\n", argv[1], argv[2], argv[3]); return 2; }
  int32_t v[9];
  size_t got;
  while ((got = fread(v, sizeof(int32_t), 9, in)) == 9) {
    const pa_bj_band_query_t q = {.ts = v[0], .R = v[1], .wmax = v[2], .count = v[3], .have_g4 = v[4], .have_pairs = v[5],
                                  .g4_wide = v[6], .mfma = v[7], .cus = v[8]};
    pa_bj_band_launch_t L;
    /* exactly WHY_LEN bytes on the heap, filled: a write beyond them is seen, and so is a text without its end */
    char* why = malloc(WHY_LEN);
    if (!why) { fprintf(stderr, "out of memory\n"); return 2; }
    memset(why, 'x', WHY_LEN);
    memset(&L, 0x7f, sizeof(L));
    const int rc = pa_bj_band_plan(&q, &L, why, WHY_LEN);
    const int32_t r[15] = {rc, why_id(why), L.family, L.ts, L.xs, L.r, L.ch, L.tiles, L.cap, L.waves, L.per_wave, L.nbuf,
                           L.lds, L.blocks, L.threads};
    fwrite(r, sizeof(int32_t), 15, out);
    free(why);
  }
  if (got != 0) { fprintf(stderr, "the queries file ends inside a record\n"); return 2; }
  for (int i = 0; i < g_nwhy; ++i) fprintf(txt, "%s\n", g_why[i]);
  fclose(in);
  if (fclose(out) || fclose(txt)) { fprintf(stderr, "writing %s / %s failed\n", argv[2], argv[3]); return 2; }
  return 0;
}
