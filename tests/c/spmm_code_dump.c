/*
 * spmm_code_dump.c -- cuts the run plan (prealps_amd/csrc/spmm_plan.c) of the matrix it is given, packs its values
 * (spmm_pack.c), codes the pack (spmm_code.c) and checks the coded form itself: for every element of every coded block
 * table[code] has the packed value's bits; entry 0 of every table is +0.0; no pattern appears twice in a table; the
 * counts of the entries behind entry 0 do not increase, ties ascend by bit pattern; a raw block has an empty table and
 * codes 0; the slack has code 0.  It prints one line of counts and writes what tests/test_spmm_code_cpu.py restates
 * with numpy to OUT:
 *
 *   int64 nblk, ncode, ntab;  int64 blk[nblk][4] = first element, end element, nown, next;
 *   int64 blk_tab_off[nblk + 1];  uint64 val[ncode] (bits);  uint16 code[ncode];  uint64 tab[ntab] (bits)
 *
 * usage: spmm_code_dump TS BUDGET FILE OUT [CUS]      (the matrix file of spmm_pack_dump.c; CUS: compute units the
 *        plan is cut for, default 1 = full blocks)
 *        spmm_code_dump fail-allocs TS BUDGET FILE      with spmm_code.c compiled -Dmalloc=t_malloc: the k-th
 *        allocation of a build fails for k = 0, 1, ...; every failure must answer -1 and leave nothing behind.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spmm_code.h"
#include "spmm_pack.h"
#include "spmm_plan.h"

static long g_allocs_left = -1;   /* >= 0: that many allocations of spmm_code.c succeed, the next one fails */
void* t_malloc(size_t n) { return (g_allocs_left >= 0 && g_allocs_left-- == 0) ? NULL : malloc(n); }

static void* must(void* p) {
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}
static void must_read(void* p, size_t elem, size_t n, FILE* f) {
  if (fread(p, elem, n, f) != n) { fprintf(stderr, "short matrix file\n"); exit(2); }
}
static void must_write(const void* p, size_t elem, size_t n, FILE* f) {
  if (fwrite(p, elem, n, f) != n) { fprintf(stderr, "short write\n"); exit(2); }
}
static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, sizeof(b)); return b; }

static int by_bits(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : x > y;
}

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s: ", name); printf(__VA_ARGS__); printf("\n"); g_failed = 1; goto out; } } while (0)

static int build(const pa_spmm_host_plan_t* pl, const pa_spmm_pack_t* pk, int ts, int budget, pa_spmm_code_t* cd) {
  return pa_spmm_code_build(pk, (const int*)pl->a[PA_PL_BLK_SLICE].p, pl->nblk, (const long long*)pl->a[PA_PL_SL_OFF].p,
                            (const int*)pl->a[PA_PL_SL_ROW0].p, (const int*)pl->a[PA_PL_SL_NROWS].p,
                            (const int*)pl->a[PA_PL_BLK_EXT_OFF].p, pl->runs, ts, budget, cd);
}

static void check_code(const char* name, const pa_spmm_host_plan_t* pl, const pa_spmm_pack_t* pk,
                       const pa_spmm_code_t* cd, int ts, int budget, const char* out_path) {
  const long long* sl_off = (const long long*)pl->a[PA_PL_SL_OFF].p;
  const int* sl_row0 = (const int*)pl->a[PA_PL_SL_ROW0].p;
  const int* sl_nrows = (const int*)pl->a[PA_PL_SL_NROWS].p;
  const int* blk_slice = (const int*)pl->a[PA_PL_BLK_SLICE].p;
  const int* blk_ext_off = (const int*)pl->a[PA_PL_BLK_EXT_OFF].p;
  const int nblk = pl->nblk;
  int64_t* blk = must(malloc(((size_t)nblk * 4 + 1) * sizeof(int64_t)));
  uint32_t* cnt = must(malloc(65536 * sizeof(uint32_t)));
  int ncoded = 0, lds = 0;
  size_t coded_elems = 0;
  CHECK(cd->nblk == nblk && cd->ncode == pk->nval_alloc && cd->tab && cd->blk_tab_off[0] == 0 &&
        (size_t)cd->blk_tab_off[nblk] == cd->ntab, "sizes");
  size_t end = 0;
  for (int b = 0; b < nblk; ++b) {
    const int s0 = blk_slice[b], s1 = blk_slice[b + 1];
    const size_t e0 = (size_t)pk->meta[4 * (size_t)(sl_off[s0] / 64) + 3], e1 = (size_t)pk->meta[4 * (size_t)(sl_off[s1] / 64) + 3];
    CHECK(e0 == end && e1 >= e0, "block %d does not follow the one before it", b);
    end = e1;
    const int nown = sl_row0[s1 - 1] + sl_nrows[s1 - 1] - sl_row0[s0], next = blk_ext_off[b + 1] - blk_ext_off[b];
    blk[4 * b] = (int64_t)e0; blk[4 * b + 1] = (int64_t)e1; blk[4 * b + 2] = nown; blk[4 * b + 3] = next;
    const int t0 = cd->blk_tab_off[b], n = cd->blk_tab_off[b + 1] - t0;
    CHECK(n >= 0 && n <= 65536, "block %d: %d table entries", b, n);
    if (n == 0) {     /* raw */
      for (size_t i = e0; i < e1; ++i) CHECK(cd->code[i] == 0, "raw block %d: code %u at %zu", b, cd->code[i], i);
      continue;
    }
    ++ncoded; coded_elems += e1 - e0;
    const int need = (nown + next + 2) * ts * 8 + 8 * n;
    CHECK(need <= budget, "block %d is coded and needs %d bytes of %d", b, need, budget);
    if (need > lds) lds = need;
    CHECK(bits_of(cd->tab[t0]) == 0, "block %d: entry 0 is not +0.0", b);
    memset(cnt, 0, (size_t)n * sizeof(uint32_t));
    for (size_t i = e0; i < e1; ++i) {
      CHECK(cd->code[i] < n, "block %d: code %u of %d at %zu", b, cd->code[i], n, i);
      CHECK(bits_of(cd->tab[t0 + cd->code[i]]) == bits_of(pk->val[i]), "block %d: element %zu decodes to other bits", b, i);
      ++cnt[cd->code[i]];
    }
    /* every step's own 0.0 has code 0 */
    for (size_t g = (size_t)(sl_off[s0] / 64); g < (size_t)(sl_off[s1] / 64); ++g)
      CHECK(cd->code[pk->meta[4 * g + 3]] == 0, "block %d: the 0.0 of step %zu has code %u", b, g, cd->code[pk->meta[4 * g + 3]]);
    for (int c = 1; c < n; ++c) {
      CHECK(cnt[c] > 0, "block %d: entry %d is used by nothing", b, c);
      CHECK(bits_of(cd->tab[t0 + c]) != 0, "block %d: +0.0 twice", b);
      if (c > 1) {
        const uint64_t p = bits_of(cd->tab[t0 + c - 1]), q = bits_of(cd->tab[t0 + c]);
        CHECK(cnt[c - 1] > cnt[c] || (cnt[c - 1] == cnt[c] && p < q), "block %d: entries %d and %d out of order", b, c - 1, c);
      }
    }
    /* no pattern twice, whatever the counts: the sorted patterns ascend strictly */
    uint64_t* sorted = must(malloc((size_t)n * sizeof(uint64_t)));
    memcpy(sorted, cd->tab + t0, (size_t)n * sizeof(uint64_t));
    qsort(sorted, (size_t)n, sizeof(uint64_t), by_bits);
    int twice = 0;
    for (int c = 1; c < n; ++c) twice |= sorted[c - 1] == sorted[c];
    free(sorted);
    CHECK(!twice, "block %d: a pattern twice", b);
  }
  CHECK(end == pk->nsteps + pk->nval, "the blocks end at %zu, the values at %zu", end, pk->nsteps + pk->nval);
  for (size_t i = end; i < cd->ncode; ++i) CHECK(cd->code[i] == 0, "slack %zu has code %u", i, cd->code[i]);
  CHECK(ncoded == cd->ncoded && coded_elems == cd->coded_elems && lds == cd->lds_bytes, "counts: %d / %d blocks, %zu / %zu elements, %d / %d bytes of LDS",
        ncoded, cd->ncoded, coded_elems, cd->coded_elems, lds, cd->lds_bytes);
  {
    FILE* f = fopen(out_path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", out_path); exit(2); }
    int64_t head[3] = {nblk, (int64_t)cd->ncode, (int64_t)cd->ntab};
    must_write(head, sizeof(int64_t), 3, f);
    must_write(blk, sizeof(int64_t), (size_t)nblk * 4, f);
    for (int b = 0; b <= nblk; ++b) { int64_t t = cd->blk_tab_off[b]; must_write(&t, sizeof(t), 1, f); }
    must_write(pk->val, sizeof(double), cd->ncode, f);
    must_write(cd->code, sizeof(uint16_t), cd->ncode, f);
    must_write(cd->tab, sizeof(double), cd->ntab, f);
    fclose(f);
  }
  printf("%s: ok runs=%d nblk=%d ncoded=%d ntab=%zu coded_elems=%zu lds=%d steps=%zu kept=%zu coded_bytes=%.0f packed_bytes=%.0f"
         " unpacked_bytes=%.0f stream_bytes=%.0f stage_cap=%d\n", name, pl->runs, nblk, cd->ncoded, cd->ntab, cd->coded_elems,
         cd->lds_bytes, pk->nsteps, pk->nval, cd->coded_bytes, pk->packed_bytes, pk->unpacked_bytes, pl->stream_bytes, pl->stage_cap);
out:
  free(blk); free(cnt);
}

static void fail_allocs(const char* name, const pa_spmm_host_plan_t* pl, const pa_spmm_pack_t* pk, int ts, int budget) {
  pa_spmm_code_t cd;
  long k = 0;
  for (;; ++k) {
    g_allocs_left = k;
    int rc = build(pl, pk, ts, budget, &cd);
    int fired = g_allocs_left < 0;
    g_allocs_left = -1;
    if (!fired) { if (rc) g_failed = 1; break; }
    int empty = !cd.code && !cd.tab && !cd.blk_tab_off && !cd.ncode && !cd.ntab && !cd.ncoded && !cd.nblk;
    if (rc != -1 || !empty) { printf("%s: failed allocation %ld gave rc=%d, %s\n", name, k, rc, empty ? "empty" : "not empty"); g_failed = 1; }
  }
  printf("%s: %s (%ld)\n", name, k >= 4 && !g_failed ? "every failed allocation handled" : "UNEXPECTED", k);
  if (k < 4) g_failed = 1;
  pa_spmm_code_free(&cd);
}

int main(int argc, char** argv) {
  int fail = argc > 1 && !strcmp(argv[1], "fail-allocs");
  if (argc != 5 && !(argc == 6 && !fail)) { fprintf(stderr, "usage: spmm_code_dump [fail-allocs] TS BUDGET FILE [OUT [CUS]]\n"); return 2; }
  const int cus = argc == 6 ? atoi(argv[5]) : 1;
  const int ts = atoi(argv[1 + fail]), budget = atoi(argv[2 + fail]);
  const char* path = argv[3 + fail];
  const char* name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int32_t head[3];
  must_read(head, sizeof(int32_t), 3, f);
  const int n = head[0], nparts = head[1], nnz = head[2];
  int* rowPos = must(malloc(((size_t)nparts + 1) * sizeof(int)));
  int* rp = must(malloc(((size_t)n + 1) * sizeof(int)));
  int* col = must(calloc((size_t)nnz + 8, sizeof(int)));
  double* v = must(malloc(((size_t)nnz + 1) * sizeof(double)));
  must_read(rowPos, sizeof(int), (size_t)nparts + 1, f);
  must_read(rp, sizeof(int), (size_t)n + 1, f);
  must_read(col, sizeof(int), (size_t)nnz, f);
  must_read(v, sizeof(double), (size_t)nnz, f);
  fclose(f);
  pa_spmm_plan_in_t in = {.m = n, .halo = 0, .part0 = 0, .part1 = nparts, .row_off = 0, .rowPos = rowPos, .rowPtr = rp,
                          .lcol = col, .val = v, .ts = ts, .cus = cus, .want_staged = -1, .want_runs = 2};
  pa_spmm_host_plan_t pl;
  pa_spmm_pack_t pk;
  memset(&pk, 0, sizeof(pk));
  if (pa_spmm_plan_build(&in, &pl) || !pl.runs) { printf("FAILED %s: no run plan\n", name); g_failed = 1; }
  else if (pa_spmm_pack_build((const double*)pl.a[PA_PL_VAL].p, (const long long*)pl.a[PA_PL_SL_OFF].p,
                              (const int*)pl.a[PA_PL_SL_LEN].p, pl.nslices, 0, &pk)) { printf("FAILED %s: no pack\n", name); g_failed = 1; }
  else if (fail) fail_allocs(name, &pl, &pk, ts, budget);
  else {
    pa_spmm_code_t cd;
    int rc = build(&pl, &pk, ts, budget, &cd);
    if (rc) { printf("FAILED %s: code rc=%d\n", name, rc); g_failed = 1; }
    else check_code(name, &pl, &pk, &cd, ts, budget, argv[4]);
    pa_spmm_code_free(&cd);
    /* a plan that is no run plan, and blocks that do not fit the pack, are refused and leave nothing behind */
    rc = pa_spmm_code_build(&pk, (const int*)pl.a[PA_PL_BLK_SLICE].p, pl.nblk, (const long long*)pl.a[PA_PL_SL_OFF].p,
                            (const int*)pl.a[PA_PL_SL_ROW0].p, (const int*)pl.a[PA_PL_SL_NROWS].p,
                            (const int*)pl.a[PA_PL_BLK_EXT_OFF].p, 0, ts, budget, &cd);
    if (rc != -2 || cd.code || cd.tab || cd.blk_tab_off) { printf("FAILED %s: no run plan gave rc=%d\n", name, rc); g_failed = 1; }
    if (pl.nblk > 1) {
      rc = pa_spmm_code_build(&pk, (const int*)pl.a[PA_PL_BLK_SLICE].p, pl.nblk - 1, (const long long*)pl.a[PA_PL_SL_OFF].p,
                              (const int*)pl.a[PA_PL_SL_ROW0].p, (const int*)pl.a[PA_PL_SL_NROWS].p,
                              (const int*)pl.a[PA_PL_BLK_EXT_OFF].p, 1, ts, budget, &cd);
      if (rc != -2 || cd.code || cd.tab || cd.blk_tab_off) { printf("FAILED %s: a block short gave rc=%d\n", name, rc); g_failed = 1; }
    }
  }
  pa_spmm_pack_free(&pk);
  pa_spmm_plan_free(&pl);
  free(rowPos); free(rp); free(col); free(v);
  return g_failed;
}
