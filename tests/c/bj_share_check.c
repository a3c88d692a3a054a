/*
 * bj_share_check.c -- runs the class pass of the block-Jacobi create (prealps_amd/csrc/bj_share.c) on cases that
 * tests/test_bj_share_cpu.py writes, and dumps what it returns for the test to compare.  No judgement here beyond
 * the sanitizers the test builds it with: usage  bj_share_check <cases in> <arrays out>.
 *
 * Cases file (native binary), case after case:
 *   int32 np, threads; uint64 hash_mask; int32 nrows[np], bw[np], eligible[np], has_band[np];
 *   float64 band[nrows * (bw + 1)] of every block with has_band, in block order (the others get no band: NULL)
 * Arrays file: records of  char name[32] ("<case>.<field>"), char type ('i' int32, 'q' int64), int64 count, then the
 * values: rc, nclass, rep[np].
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
  int threads;
  uint64_t mask;
  get(&threads, sizeof(int), 1);
  get(&mask, sizeof(mask), 1);
  int* nrows = get_ints((size_t)np);
  int* bw = get_ints((size_t)np);
  int* el = get_ints((size_t)np);
  int* has = get_ints((size_t)np);
  char* eligible = must(malloc((size_t)np + 1));
  double** bands = must(calloc((size_t)np + 1, sizeof(double*)));
  int* rep = must(malloc(((size_t)np + 1) * sizeof(int)));
  for (int p = 0; p < np; ++p) {
    eligible[p] = (char)el[p];
    if (!has[p]) continue;
    const size_t len = (size_t)nrows[p] * ((size_t)bw[p] + 1);
    bands[p] = must(malloc((len ? len : 1) * sizeof(double)));      /* exactly the band: a read beyond it is seen */
    get(bands[p], sizeof(double), len);
  }
  const pa_bj_share_in_t in = {.np = np, .nrows = nrows, .bw = bw, .eligible = eligible, .bands = bands,
                               .threads = threads, .hash_mask = mask};
  int nclass = -1;
  const int rc = pa_bj_share_classes(&in, rep, &nclass);
  put_int("rc", rc); put_int("nclass", nclass); put("rep", 'i', rep, (size_t)np);
  for (int p = 0; p < np; ++p) free(bands[p]);
  free(nrows); free(bw); free(el); free(has); free(eligible); free(bands); free(rep);
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
