/* Stand-alone run of pa_ecg_x_mode (prealps_amd/csrc/ecg_plan.c; tests/test_x_defer_cpu.py).
 *   rule   one line per input: on pending another_step_follows mode
 *   trace  calls of preAlps_ECGAdvance as solve_first_step and ecg_advance_loop drive the rule: three calls of 1, 2, 3 or
 *          5 steps each, the switch off and on, the stopping test firing at one step of the whole sequence (or at none,
 *          -1).  One line per case: on n0 n1 n2 stop_at, then the events in order -- E / S / B: a row pass of that mode,
 *          F: pa_k_flush_x, |0 or |1: a call returns with nothing / something owed.
 *   solve  preAlps_ECGSolve: every step is followed by another unless the test fires, which it does at step stop_at
 *          (0 .. 8).  One line per case: on stop_at, then the events as above. */
#include <stdio.h>
#include <string.h>

#include "ecg_plan.h"

static void rule(void) {
  for (int on = 0; on < 2; ++on) for (int pending = 0; pending < 2; ++pending) for (int ahead = 0; ahead < 2; ++ahead)
    printf("%d %d %d %d\n", on, pending, ahead, pa_ecg_x_mode(on, pending, ahead));
}

static void trace(void) {
  static const int sizes[4] = {1, 2, 3, 5};
  for (int on = 0; on < 2; ++on) for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) for (int c = 0; c < 4; ++c) {
    const int n[3] = {sizes[a], sizes[b], sizes[c]}, total = n[0] + n[1] + n[2];
    for (int stop_at = -1; stop_at < total; ++stop_at) {
      int pending = 0, step = 0;
      printf("%d %d %d %d %d ", on, n[0], n[1], n[2], stop_at);
      for (int call = 0; call < 3; ++call) {
        for (int done = 0; done < n[call]; ++done, ++step) {
          const int mode = pa_ecg_x_mode(on, pending, done + 1 < n[call]);
          putchar(mode == PA_ECG_X_SKIP ? 'S' : mode == PA_ECG_X_BOTH ? 'B' : mode == PA_ECG_X_EVERY ? 'E' : '?');
          pending = mode == PA_ECG_X_SKIP;
          if (step == stop_at && pending) { putchar('F'); pending = 0; }      /* (then the restart, inside the call) */
        }
        printf("|%d", pending);
      }
      printf("\n");
    }
  }
}

static void solve(void) {
  for (int on = 0; on < 2; ++on) for (int stop_at = 0; stop_at < 9; ++stop_at) {
    int pending = 0;
    printf("%d %d ", on, stop_at);
    for (int step = 0; step <= stop_at; ++step) {
      const int mode = pa_ecg_x_mode(on, pending, 1);
      putchar(mode == PA_ECG_X_SKIP ? 'S' : mode == PA_ECG_X_BOTH ? 'B' : mode == PA_ECG_X_EVERY ? 'E' : '?');
      pending = mode == PA_ECG_X_SKIP;
      if (step == stop_at && pending) { putchar('F'); pending = 0; }
    }
    printf("|%d\n", pending);
  }
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "rule")) rule();
  else if (argc == 2 && !strcmp(argv[1], "trace")) trace();
  else if (argc == 2 && !strcmp(argv[1], "solve")) solve();
  else { fprintf(stderr, "usage: %s rule|trace|solve\n", argv[0]); return 2; }
  return 0;
}
