/*
 * bj_pair_check.c -- runs the pair-task builder of the block-Jacobi create (prealps_amd/csrc/bj_share.c:
 * pa_bj_pair_tasks) on cases that tests/test_bj_pair_cpu.py writes, and dumps what it returns for the test to compare.
 * No judgement here beyond the sanitizers the test builds it with: usage  bj_pair_check <cases in> <arrays out>.
 *
 * Cases file (native binary), case after case:
 *   int32 np, count; int32 rep[np], nrows[np], bw[np]; int32 list[count]
 * Arrays file: records of  char name[32] ("<case>.<field>"), char type ('i' int32, 'q' int64), int64 count, then the
 * values: rc, ntasks, paired, tasks[2 * ntasks].
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_share.h"

static FILE* g_in;
static FILE* g_out;
static int g_case;

static void* must(void* p) {
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}
static void get(void* p, size_t size, size_t n) {
  if (n && fread(p, size, n, g_in) != n) { fprintf(stderr, "case %d: the cases file ends early\n", g_case); exit(2); }
}
/* exactly n ints (one when n = 0): a read or a write beyond them is seen */
static int* get_ints(size_t n) { int* p = must(malloc((n ? n : 1) * sizeof(int))); get(p, sizeof(int), n); return p; }

static void put(const char* field, char type, const void* p, size_t n) {
  char name[32];
  const int64_t cnt = (int64_t)n;
  memset(name, 0, sizeof(name));
  snprintf(name, sizeof(name), "%d.%s", g_case, field);
  fwrite(name, 1, sizeof(name), g_out); fwrite(&type, 1, 1, g_out); fwrite(&cnt, sizeof(cnt), 1, g_out);
  if (n) fwrite(p, type == 'i' ? 4 : 8, n, g_out);
}
static void put_int(const char* field, long long v) { int64_t x = v; put(field, 'q', &x, 1); }

static void one_case(int np) {
  int count;
  get(&count, sizeof(int), 1);
  if (count < 0) { fprintf(stderr, "case %d: a list of %d\n", g_case, count); exit(2); }
  int* rep = get_ints((size_t)np);
  int* nrows = get_ints((size_t)np);
  int* bw = get_ints((size_t)np);
  int* list = get_ints((size_t)count);
  int* tasks = must(malloc((count ? 2 * (size_t)count : 1) * sizeof(int)));
  memset(tasks, 0x7f, (count ? 2 * (size_t)count : 1) * sizeof(int));
  int ntasks = -1, paired = -1;
  const int rc = pa_bj_pair_tasks(np, list, count, rep, nrows, bw, tasks, &ntasks, &paired);
  put_int("rc", rc); put_int("ntasks", ntasks); put_int("paired", paired);
  put("tasks", 'i', tasks, ntasks > 0 ? 2 * (size_t)ntasks : 0);
  fflush(g_out);
  free(rep); free(nrows); free(bw); free(list); free(tasks);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <cases in> <arrays out>\n", argv[0]); return 2; }
  g_in = fopen(argv[1], "rb");
  g_out = fopen(argv[2], "wb");
  if (!g_in || !g_out) { fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]); return 2; }
  int np;
  for (g_case = 0; fread(&np, sizeof(int), 1, g_in) == 1; ++g_case) {
    if (np < 0) { fprintf(stderr, "case %d: %d blocks\n", g_case, np); return 2; }
    one_case(np);
  }
  fclose(g_in);
  if (fclose(g_out)) { fprintf(stderr, "writing %s failed\n", argv[2]); return 2; }
  return 0;
}
