/* Stand-alone run of prealps_amd/csrc/ecg_plan.c (tests/test_ecg_plan_cpu.py): prints, one case per line, the
 * inputs and what the unit answers -- `layout`: every offset of the solver's pool; `switches`: the decisions of a
 * reset.  An absent region prints as -1. */
#include <stdio.h>
#include <string.h>

#include "ecg_plan.h"

static long long off(size_t v) { return v == PA_ECG_ABSENT ? -1LL : (long long)v; }

static void layout_cases(void) {
  static const int Ts[7] = {1, 2, 3, 4, 8, 12, 16}, tss[7] = {2, 2, 4, 4, 8, 16, 16};
  static const int ms[4] = {0, 1, 5, 1000}, spmm[2] = {0, 7}, bj[2] = {0, 9}, Gs[2] = {40, 264}, Ss[2] = {9, 17};
  for (int a = 0; a < 7; ++a) for (int alg = 0; alg < 3; ++alg) for (int b = 0; b < 4; ++b)
    for (int c = 0; c < 2; ++c) for (int d = 0; d < 2; ++d) for (int e = 0; e < 2; ++e) for (int f = 0; f < 2; ++f) {
      const pa_ecg_pool_in_t in = {.m = ms[b], .T = Ts[a], .ts = tss[a], .ortho_alg = alg, .spmm_cap = spmm[c],
                                   .bj_cap = bj[d], .G = Gs[e], .S = Ss[f]};
      pa_ecg_pool_t o;
      memset(&o, 0x5a, sizeof(o));
      pa_ecg_pool_layout(&in, &o);
      printf("%d %d %d %d %d %d %d %d", in.m, in.T, in.ts, in.ortho_alg, in.spmm_cap, in.bj_cap, in.G, in.S);
      const size_t all[22] = {o.v[0], o.v[1], o.av[0], o.av[1], o.z, o.r, o.x, o.F, o.alpha, o.beta, o.mu, o.rtr, o.q,
                              o.res2, o.uu, o.partials, o.rtr_part, o.spmm_parts, o.bj_parts, o.grp, o.sys_part,
                              o.pool_doubles};
      for (int i = 0; i < 22; ++i) printf(" %lld", off(all[i]));
      printf("\n");
    }
}

static void switch_cases(void) {
  static const int enl[4] = {1, 2, 4, 8}, world[3] = {1, 1, 8}, loop[3] = {0, 1, 0};
  for (int alg = 0; alg < 3; ++alg) for (int bs = 0; bs < 2; ++bs) for (int e = 0; e < 4; ++e)
    for (int nrhs = 1; nrhs <= 2; ++nrhs) for (int guess = 0; guess < 2; ++guess) for (int metric = 0; metric < 2; ++metric)
      for (int w = 0; w < 3; ++w) for (int timing = 0; timing < 2; ++timing) for (int fuse = 0; fuse < 2; ++fuse)
        for (int ln = 0; ln < 2; ++ln) for (int ls = 0; ls < 2; ++ls) for (int g = 0; g < 3; ++g) for (int poll = -1; poll < 2; ++poll) {
          const pa_ecg_switch_in_t in = {.ortho_alg = alg, .bs_red = bs, .enlFac = enl[e], .nrhs = nrhs, .guess = guess,
                                         .metric = metric, .world = world[w], .loopback = loop[w], .timing = timing,
                                         .fuse = fuse, .lazy_norm = ln, .lazy_stop = ls, .graphs = g,
                                         .poll = poll};
          pa_ecg_switch_t o;
          memset(&o, 0x5a, sizeof(o));
          pa_ecg_switches(&in, &o);
          printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d\n", alg, bs, enl[e], nrhs, guess, metric,
                 world[w], loop[w], timing, fuse, ln, ls, g, poll, o.rotate, o.fuse, o.lazy_norm, o.lazy_stop,
                 o.use_graphs, o.poll, o.ride);
        }
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) layout_cases();
  else if (argc == 2 && !strcmp(argv[1], "switches")) switch_cases();
  else { fprintf(stderr, "usage: %s layout|switches\n", argv[0]); return 2; }
  return 0;
}
