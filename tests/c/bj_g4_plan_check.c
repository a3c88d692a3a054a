/*
 * bj_g4_plan_check.c -- runs the launch planner of the band block solve (prealps_amd/csrc/bj_g4_plan.c: pa_bj_g4_plan)
 * on the queries that tests/test_bj_g4_plan_cpu.py writes, and dumps the plans for the test to compare.  No judgement
 * here beyond the sanitizers the test builds it with: usage  bj_g4_plan_check <queries in> <plans out> <reasons out>.
 *
 * Queries file (native binary): records of 14 int32 in the order of pa_bj_g4_query_t --
 *   count wmax bmax xs ncol bits gram cus ring_env pair_mode pair_intact have_tasks ntasks paired
 * Plans file: one record of 18 int32 per query --
 *   rc why kind nt nc dq occ gp bits ring waves per_wave lds blocks last[0..3]
 * `why` = line (from 0) of the reasons file that holds the text the planner left (an empty line for a plan it made):
 * every distinct text is written once, in the order of its first appearance.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_g4_plan.h"

#define WHY_LEN 128
#define WHY_MAX 1024

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
  int32_t v[14];
  size_t got;
  while ((got = fread(v, sizeof(int32_t), 14, in)) == 14) {
    const pa_bj_g4_query_t q = {.count = v[0], .wmax = v[1], .bmax = v[2], .xs = v[3], .ncol = v[4], .bits = v[5],
                                .gram = v[6], .cus = v[7], .ring_env = v[8], .pair_mode = v[9], .pair_intact = v[10],
                                .have_tasks = v[11], .ntasks = v[12], .paired = v[13]};
    pa_bj_g4_launch_t L;
    /* exactly WHY_LEN bytes on the heap, filled: a write beyond them is seen, and so is a text without its end */
    char* why = malloc(WHY_LEN);
    if (!why) { fprintf(stderr, "out of memory\n"); return 2; }
    memset(why, 'x', WHY_LEN);
    memset(&L, 0x7f, sizeof(L));
    const int rc = pa_bj_g4_plan(&q, &L, why, WHY_LEN);
    const int32_t r[18] = {rc, why_id(why), L.kind, L.nt, L.nc, L.dq, L.occ, L.gp, L.bits, L.ring, L.waves, L.per_wave,
                           L.lds, L.blocks, L.last[0], L.last[1], L.last[2], L.last[3]};
    fwrite(r, sizeof(int32_t), 18, out);
    free(why);
  }
  if (got != 0) { fprintf(stderr, "the queries file ends inside a record\n"); return 2; }
  for (int i = 0; i < g_nwhy; ++i) fprintf(txt, "%s\n", g_why[i]);
  fclose(in);
  if (fclose(out) || fclose(txt)) { fprintf(stderr, "writing %s / %s failed\n", argv[2], argv[3]); return 2; }
  return 0;
}
