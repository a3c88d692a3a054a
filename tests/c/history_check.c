/* Stand-alone run of prealps_amd/csrc/ecg_history.c (tests/test_ecg_history_cpu.py): reads a script of commands from
 * standard input, drives the unit with it and prints what the unit answers; numbers travel as hex floats.
 *   I cap                          pa_hist_init                      -> "I status"
 *   A q K <K*q DO> <q*q DN>        pa_hist_append (column major)     -> "A status count head slot_0 .. slot_q-1", then
 *                                                                       "G" and the 16 x 16 entries of G
 *   P q rtol <count*q g>           pa_hist_project (logical order)   -> "P status rank", count*q coefficients, q captured
 *   S K q rtol <K*K Gs> <K*q gs>   pa_hist_factor_solve              -> "S rank piv_0 .. piv_rank-1", K*q coefficients
 *   L                              the slots in logical order        -> "L slot_0 .. slot_count-1 | -1 -1"
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "ecg_history.h"

static int read_doubles(double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%lf", v + i) != 1) return 1;
  return 0;
}

int main(void) {
  pa_hist_t h;
  char cmd;
  double a[PA_HIST_MAX * PA_HIST_MAX], b[PA_HIST_MAX * PA_HIST_MAX], c[PA_HIST_MAX * PA_HIST_MAX];
  if (pa_hist_init(&h, 1) != PA_HIST_OK) return 2;
  /* out of range: refused, and the ring is as it was */
  if (pa_hist_init(&h, 0) != PA_HIST_BAD_ARGS || pa_hist_init(&h, PA_HIST_MAX + 1) != PA_HIST_BAD_ARGS || h.cap != 1) return 2;
  if (pa_hist_capacity_ok(0) || !pa_hist_capacity_ok(1) || !pa_hist_capacity_ok(16) || pa_hist_capacity_ok(17)) return 2;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'I') {
      int cap;
      if (scanf("%d", &cap) != 1) return 3;
      printf("I %d\n", pa_hist_init(&h, cap));
    } else if (cmd == 'A') {
      int q, K, slots[PA_HIST_MAX];
      if (scanf("%d %d", &q, &K) != 2 || q < 1 || q > PA_HIST_MAX || K != h.count) return 3;
      if (read_doubles(a, K * q) || read_doubles(b, q * q)) return 3;
      const int st = pa_hist_append(&h, q, a, K > 0 ? K : 1, b, q, slots);
      printf("A %d %d %d", st, h.count, h.head);
      for (int j = 0; j < q; ++j) printf(" %d", st ? -2 : slots[j]);
      printf("\nG");
      for (int e = 0; e < PA_HIST_MAX * PA_HIST_MAX; ++e) printf(" %a", h.G[e]);
      printf("\n");
    } else if (cmd == 'P') {
      int q, rank = -1;
      double rtol, cap[PA_HIST_MAX];
      if (scanf("%d %lf", &q, &rtol) != 2 || q < 1 || q > PA_HIST_MAX) return 3;
      if (read_doubles(a, h.count * q)) return 3;
      const int st = pa_hist_project(&h, q, a, rtol, c, &rank, cap);
      printf("P %d %d", st, rank);
      for (int e = 0; !st && e < h.count * q; ++e) printf(" %a", c[e]);
      for (int j = 0; !st && j < q; ++j) printf(" %a", cap[j]);
      printf("\n");
    } else if (cmd == 'S') {
      int K, q, piv[PA_HIST_MAX];
      double rtol;
      if (scanf("%d %d %lf", &K, &q, &rtol) != 3 || K < 1 || K > PA_HIST_MAX || q < 1 || q > PA_HIST_MAX) return 3;
      if (read_doubles(a, K * K) || read_doubles(b, K * q)) return 3;
      const int rank = pa_hist_factor_solve(K, a, q, b, rtol, c, piv);
      printf("S %d", rank);
      for (int i = 0; i < rank; ++i) printf(" %d", piv[i]);
      for (int e = 0; e < K * q; ++e) printf(" %a", c[e]);
      printf("\n");
    } else if (cmd == 'L') {
      printf("L");
      for (int i = 0; i < h.count; ++i) printf(" %d", pa_hist_slot(&h, i));
      printf(" | %d %d\n", pa_hist_slot(&h, -1), pa_hist_slot(&h, h.count));
    } else return 4;
  }
  return 0;
}
