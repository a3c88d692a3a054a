/* Stand-alone run of pa_hist_red_layout (prealps_amd/csrc/ecg_history.c; tests/test_history_ranks_cpu.py): prints, for
 * every entry and every K and q it is asked for, "entry K q status off_a rows_a cols_a off_b rows_b cols_b words", and
 * checks on its own what must hold whatever the numbers are: a refused shape leaves the layout untouched, the blocks lie
 * behind word 0, inside the buffer and apart, and filling them through the offsets writes no word twice and none
 * outside [1, words). */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "ecg_history.h"

int main(void) {
  double red[PA_HIST_RED_WORDS];
  for (int entry = -1; entry <= 3; ++entry)
    for (int K = -1; K <= PA_HIST_MAX + 1; ++K)
      for (int q = -1; q <= PA_HIST_MAX + 1; ++q) {
        pa_hist_red_t l;
        memset(&l, 0x5a, sizeof(l));
        const pa_hist_red_t before = l;
        const int st = pa_hist_red_layout(entry, K, q, &l);
        if (st != PA_HIST_OK) {
          if (st != PA_HIST_BAD_ARGS || memcmp(&l, &before, sizeof(l)) != 0) return 2;      /* (l untouched) */
          printf("%d %d %d %d\n", entry, K, q, st);
          continue;
        }
        printf("%d %d %d %d %d %d %d %d %d %d %d\n", entry, K, q, st, l.off_a, l.rows_a, l.cols_a, l.off_b, l.rows_b, l.cols_b,
               l.words);
        const int na = l.rows_a * l.cols_a, nb = l.rows_b * l.cols_b;
        if (l.off_a < 1 || l.off_b < l.off_a + na || l.words < l.off_b + nb || l.words > PA_HIST_RED_WORDS) return 4;
        /* written through the offsets: na + nb words of [1, words), each once, nothing else */
        for (int w = 0; w < PA_HIST_RED_WORDS; ++w) red[w] = 0.0;
        for (int j = 0; j < l.cols_a; ++j) for (int i = 0; i < l.rows_a; ++i) red[l.off_a + i + l.rows_a * j] += 1.0;
        for (int j = 0; j < l.cols_b; ++j) for (int i = 0; i < l.rows_b; ++i) red[l.off_b + i + l.rows_b * j] += 1.0;
        double sum = 0.0;
        for (int w = 0; w < PA_HIST_RED_WORDS; ++w) {
          if (red[w] != 0.0 && (red[w] != 1.0 || w < 1 || w >= l.words)) return 5;
          sum += red[w];
        }
        if (sum != (double)(na + nb)) return 5;
      }
  if (pa_hist_red_layout(PA_HIST_RED_PROJECT, 1, 1, NULL) != PA_HIST_BAD_ARGS) return 6;
  return 0;
}
