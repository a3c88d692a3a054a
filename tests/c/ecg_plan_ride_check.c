/* Stand-alone run of pa_ecg_switches (prealps_amd/csrc/ecg_plan.c) for tests/test_ecg_plan_ride_cpu.py: the inputs of
 * the switch table of ecg_plan_check.c, one case per line, followed by the seven decisions that table prints and, last,
 * ride_sys.  The output struct is filled with a pattern first, so a field the unit leaves unwritten shows. */
#include <stdio.h>
#include <string.h>

#include "ecg_plan.h"

int main(void) {
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
          printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d %d\n", alg, bs, enl[e], nrhs, guess, metric,
                 world[w], loop[w], timing, fuse, ln, ls, g, poll, o.rotate, o.fuse, o.lazy_norm, o.lazy_stop,
                 o.use_graphs, o.poll, o.ride, o.ride_sys);
        }
  /* ride_sys is the last field: the ones in front of it keep their place */
  if (sizeof(pa_ecg_switch_t) != 8 * sizeof(int)) { fprintf(stderr, "pa_ecg_switch_t has grown by more than ride_sys\n"); return 1; }
  {
    pa_ecg_switch_t o;
    if ((char*)&o.ride_sys - (char*)&o != 7 * (int)sizeof(int)) { fprintf(stderr, "ride_sys is not the last field\n"); return 1; }
  }
  return 0;
}
