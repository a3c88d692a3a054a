/* Stand-alone run of prealps_amd/csrc/ecg_refine.c (tests/test_refine_cpu.py): prints, one case per line, the inputs
 * and what the unit answers.
 *   ratio:   k, then k pairs res thr (hex floats), then the ratio (hex float; "inf" for +Inf)
 *   verdict: q q_prev (hex floats) pass max_passes iters_used max_iter -> verdict keep_prev
 *   chain:   a scripted solve driven as preAlps_ECGSolveSystemRefined drives it -- per pass p the ratio its start
 *            finds and the iterations it would take if it got as many as it wanted; prints per script
 *            max_passes max_iter n_passes status keep_prev used, then the iterations every pass got */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "ecg_refine.h"

static void ratio_cases(void) {
  static const double res[][4] = {{3.0}, {0.0}, {1.0, 8.0, 2.0}, {1.0, NAN, 2.0}, {1.0, 2.0, INFINITY}, {1.0, 2.0}, {-1.0, 2.0},
                                  {5e-324, 1e308, 1.0, 1.0}};
  static const double thr[][4] = {{2.0}, {2.0}, {2.0, 4.0, 0.5}, {2.0, 4.0, 0.5}, {2.0, 4.0, 0.5}, {2.0, 0.0}, {2.0, 4.0},
                                  {1.0, 1e-10, 3.0, 1.0}};
  static const int ks[] = {1, 1, 3, 3, 3, 2, 2, 4};
  for (int c = 0; c < 8; ++c) {
    printf("%d", ks[c]);
    for (int j = 0; j < ks[c]; ++j) printf(" %a %a", res[c][j], thr[c][j]);
    printf(" %a\n", pa_refine_ratio(ks[c], res[c], thr[c]));
  }
}

static void verdict_cases(void) {
  /* around 1 and around the halving edge: q_prev / 2 one ulp either side */
  static const double qs[] = {0.0, 0.5, 1.0, 0x1.0000000000001p+0, 2.0, 0x1.fffffffffffffp+0, 0x1.0000000000001p+1, 3.0, 1e3,
                              INFINITY};
  static const double qp[] = {1.5, 2.0, 4.0, 0x1.0000000000001p+2, 6.0, 1e3, INFINITY};
  static const int mps[] = {1, 2, 4, 16}, used[] = {0, 99, 100, 101};
  for (unsigned a = 0; a < sizeof(qs) / sizeof(*qs); ++a) for (unsigned b = 0; b < sizeof(qp) / sizeof(*qp); ++b)
    for (int c = 0; c < 4; ++c) for (int pass = 1; pass <= mps[c]; ++pass) for (int d = 0; d < 4; ++d) {
      int keep = 0x5a5a;
      const int v = pa_refine_verdict(qs[a], qp[b], pass, mps[c], used[d], 100, &keep);
      printf("%a %a %d %d %d %d %d %d\n", qs[a], qp[b], pass, mps[c], used[d], 100, v, keep);
    }
  /* keep_prev may be NULL */
  printf("%d\n", pa_refine_verdict(3.0, 2.0, 2, 4, 0, 100, NULL));
}

typedef struct { int max_passes, max_iter, n; double q[18]; int want[18]; } script_t;
static void chain_cases(void) {
  static const script_t S[] = {
    {4, 100, 2, {0, 0.7}, {30}},                                  /* one pass, converged at the start of pass 1 */
    {4, 100, 3, {0, 9.0, 0.2}, {30, 5}},                          /* the repair: two passes */
    {1, 100, 2, {0, 9.0}, {30}},                                  /* out of passes after pass 0 */
    {3, 100, 4, {0, 64.0, 8.0, 2.0}, {10, 10, 10}},               /* out of passes with every pass halving */
    {4, 100, 3, {0, 9.0, 4.5}, {30, 5}},                          /* exactly halved: goes on, pass 2 runs ... */
    {4, 100, 4, {0, 9.0, 4.5, 0x1.2000000000001p+1}, {30, 5, 5}}, /* ... and one ulp above half stops it */
    {4, 100, 3, {0, 9.0, 12.0}, {30, 5}},                         /* a pass that made it worse: the iterate before it */
    {4, 100, 3, {0, 9.0, 3.0}, {60, 70}},                         /* the budget: pass 1 gets 40, then none is left */
    {16, 1000, 17, {0, 65536.0, 32768.0, 16384.0, 8192.0, 4096.0, 2048.0, 1024.0, 512.0, 256.0, 128.0, 64.0, 32.0, 16.0,
                    8.0, 4.0, 2.0}, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}},   /* sixteen passes */
    {4, 30, 2, {0, 9.0}, {30}},                                   /* pass 0 alone uses the budget */
  };
  for (unsigned s = 0; s < sizeof(S) / sizeof(*S); ++s) {
    const script_t* c = &S[s];
    int used = 0, status = PA_REFINE_CONTINUE, keep = 0, got[17] = {0}, p;
    double q_prev = 0.0;
    for (p = 0; p < c->n; ++p) {
      if (p > 0) {
        status = pa_refine_verdict(c->q[p], q_prev, p, c->max_passes, used, c->max_iter, &keep);
        if (status != PA_REFINE_CONTINUE) break;
        q_prev = c->q[p];
      }
      const int left = c->max_iter - used;
      got[p] = c->want[p] < left ? c->want[p] : left;
      used += got[p];
    }
    printf("%d %d %d %d %d %d ", c->max_passes, c->max_iter, p, status, keep, used);
    for (int i = 0; i < p; ++i) printf(" %d", got[i]);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "ratio")) ratio_cases();
  else if (argc == 2 && !strcmp(argv[1], "verdict")) verdict_cases();
  else if (argc == 2 && !strcmp(argv[1], "chain")) chain_cases();
  else if (argc == 2 && !strcmp(argv[1], "passes")) {
    for (int mp = -1; mp <= 18; ++mp) printf("%d %d\n", mp, pa_refine_passes_ok(mp));
  } else { fprintf(stderr, "usage: %s ratio|verdict|chain|passes\n", argv[0]); return 2; }
  return 0;
}
