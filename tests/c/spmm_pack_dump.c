/*
 * spmm_pack_dump.c -- cuts the run plan (prealps_amd/csrc/spmm_plan.c) of the matrices it is given, packs the
 * plan's value array (prealps_amd/csrc/spmm_pack.c) and checks the packed form itself: unpacked through masks and
 * offsets it is the value array again, bit for bit; pack_pos is strictly increasing and names exactly the places
 * the masks name; every step's part starts with 0.0 and the array ends in zeros; lanes beyond a slice's rows have
 * clear bits.  One line per matrix with the counts tests/test_spmm_pack_cpu.py holds against the matrix.
 *
 * A matrix file: int32 n, nparts, nnz; int32 rowPos[nparts + 1]; int32 rowPtr[n + 1]; int32 col[nnz]; double
 * val[nnz] -- one panel of all rows, the parts contiguous.
 *
 * With spmm_pack.c compiled -Dmalloc=t_malloc, `spmm_pack_dump fail-allocs FILE...` lets the k-th allocation of
 * a pack fail for k = 0, 1, ...: every failure must answer -1 and leave an empty pack, and -- the sanitizers
 * watch -- neither leak nor touch freed memory.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spmm_pack.h"
#include "spmm_plan.h"

static long g_allocs_left = -1;   /* >= 0: that many allocations of spmm_pack.c succeed, the next one fails */
void* t_malloc(size_t n) { return (g_allocs_left >= 0 && g_allocs_left-- == 0) ? NULL : malloc(n); }

static void* must(void* p) {
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}
static void must_read(void* p, size_t elem, size_t n, FILE* f) {
  if (fread(p, elem, n, f) != n) { fprintf(stderr, "short matrix file\n"); exit(2); }
}
static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, sizeof(b)); return b; }
static int popc(uint64_t m) { int c = 0; for (; m; m &= m - 1) ++c; return c; }

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s: ", name); printf(__VA_ARGS__); printf("\n"); g_failed = 1; return; } } while (0)

static void check_pack(const char* name, const pa_spmm_host_plan_t* pl, const pa_spmm_pack_t* pk) {
  const double* val = (const double*)pl->a[PA_PL_VAL].p;
  const long long* sl_off = (const long long*)pl->a[PA_PL_SL_OFF].p;
  const int* sl_len = (const int*)pl->a[PA_PL_SL_LEN].p;
  const int* sl_nrows = (const int*)pl->a[PA_PL_SL_NROWS].p;
  const int* blk_slice = (const int*)pl->a[PA_PL_BLK_SLICE].p;
  const size_t n = pl->a[PA_PL_VAL].n;
  CHECK(pk->nsteps * 192 == n, "steps %zu against %zu values", pk->nsteps, n);
  CHECK(pk->nval_alloc == pk->nsteps + pk->nval + PA_SPMM_PACK_SLACK && pk->nsteps_alloc == pk->nsteps + 1, "sizes");
  /* unpack */
  double* un = must(malloc((n ? n : 1) * sizeof(double)));
  size_t j = 0, empty_masks = 0, negzeros = 0;
  for (size_t g = 0; g < pk->nsteps; ++g) {
    const uint64_t* q = pk->meta + 4 * g;
    if (q[3] != g + j || bits_of(pk->val[q[3]]) != 0) { free(un); CHECK(0, "step %zu starts at %llu, not at %zu with 0.0", g, (unsigned long long)q[3], g + j); }
    size_t first = q[3] + 1;
    for (int p = 0; p < 3; ++p) {
      empty_masks += q[p] == 0;
      for (int i = 0; i < 64; ++i) {
        const size_t s = g * 192 + (size_t)p * 64 + (size_t)i;
        if (!((q[p] >> i) & 1)) { un[s] = pk->val[q[3]]; continue; }      /* what a lane without a value reads */
        const size_t at = first + (size_t)popc(q[p] & (((uint64_t)1 << i) - 1));
        un[s] = pk->val[at];
        if (bits_of(un[s]) == 0 || pk->pos[j] != s || (j && pk->pos[j] <= pk->pos[j - 1])) {
          free(un);
          CHECK(0, "kept value %zu (slot %zu): a +0.0, or pack_pos %u out of order", j, s, pk->pos[j]);
        }
        negzeros += bits_of(un[s]) == 0x8000000000000000ULL;
        ++j;
      }
      first += (size_t)popc(q[p]);
    }
  }
  int same = j == pk->nval && memcmp(un, val, n * sizeof(double)) == 0;
  free(un);
  CHECK(same, "the unpacked values are not the plan's (%zu kept, %zu counted)", pk->nval, j);
  const uint64_t* spare = pk->meta + 4 * pk->nsteps;
  CHECK(!spare[0] && !spare[1] && !spare[2] && spare[3] == pk->nsteps + pk->nval, "the spare step");
  for (size_t i = pk->nsteps + pk->nval; i < pk->nval_alloc; ++i) CHECK(bits_of(pk->val[i]) == 0, "slack %zu", i);
  /* lanes beyond the slice's rows */
  int min_rows = 64, max_blk = 0;
  for (int s = 0; s < pl->nslices; ++s) {
    if (sl_nrows[s] < min_rows) min_rows = sl_nrows[s];
    const uint64_t beyond = sl_nrows[s] >= 64 ? 0 : ~(uint64_t)0 << sl_nrows[s];
    for (int k = 0; k < sl_len[s]; ++k)
      for (int p = 0; p < 3; ++p)
        CHECK(!(pk->meta[4 * ((size_t)(sl_off[s] / 64) + (size_t)k) + p] & beyond), "slice %d step %d: a lane beyond the rows has a value", s, k);
  }
  for (int b = 0; b < pl->nblk; ++b) if (blk_slice[b + 1] - blk_slice[b] > max_blk) max_blk = blk_slice[b + 1] - blk_slice[b];
  CHECK(pk->unpacked_bytes == 8.0 * (double)n && pk->packed_bytes == 8.0 * (double)(pk->nsteps + pk->nval) + 32.0 * (double)pk->nsteps, "byte counts");
  printf("%s: ok runs=%d nslices=%d nblk=%d max_block_slices=%d min_slice_rows=%d steps=%zu stored=%zu kept=%zu"
         " empty_masks=%zu negzeros=%zu packed_bytes=%.0f unpacked_bytes=%.0f\n", name, pl->runs, pl->nslices, pl->nblk,
         max_blk, min_rows, pk->nsteps, n, pk->nval, empty_masks, negzeros, pk->packed_bytes, pk->unpacked_bytes);
}

static void fail_allocs(const char* name, const pa_spmm_host_plan_t* pl) {
  pa_spmm_pack_t pk;
  long k = 0;
  for (;; ++k) {
    g_allocs_left = k;
    int rc = pa_spmm_pack_build((const double*)pl->a[PA_PL_VAL].p, (const long long*)pl->a[PA_PL_SL_OFF].p,
                                (const int*)pl->a[PA_PL_SL_LEN].p, pl->nslices, 1, &pk);
    int fired = g_allocs_left < 0;
    g_allocs_left = -1;
    if (!fired) { if (rc) g_failed = 1; break; }
    int empty = !pk.meta && !pk.val && !pk.pos && !pk.nval && !pk.nsteps;
    if (rc != -1 || !empty) { printf("%s: failed allocation %ld gave rc=%d, pack %s\n", name, k, rc, empty ? "empty" : "not empty"); g_failed = 1; }
  }
  printf("%s: %s (%ld)\n", name, k == 3 ? "every failed allocation handled" : "UNEXPECTED NUMBER OF ALLOCATIONS", k);
  if (k != 3) g_failed = 1;
  pa_spmm_pack_free(&pk);
}

static void one_file(const char* path, int fail) {
  const char* name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
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
                          .lcol = col, .val = v, .ts = 4, .cus = 1, .want_staged = -1, .want_runs = 2};   /* (one CU: full blocks) */
  pa_spmm_host_plan_t pl;
  if (pa_spmm_plan_build(&in, &pl) || !pl.runs) { printf("FAILED %s: no run plan\n", name); g_failed = 1; }
  else if (fail) fail_allocs(name, &pl);
  else {
    pa_spmm_pack_t pk;
    int rc = pa_spmm_pack_build((const double*)pl.a[PA_PL_VAL].p, (const long long*)pl.a[PA_PL_SL_OFF].p,
                                (const int*)pl.a[PA_PL_SL_LEN].p, pl.nslices, 1, &pk);
    if (rc) { printf("FAILED %s: pack rc=%d\n", name, rc); g_failed = 1; }
    else check_pack(name, &pl, &pk);
    pa_spmm_pack_free(&pk);
    /* slices that are not whole steps behind each other are refused, and leave nothing behind */
    long long* off = (long long*)pl.a[PA_PL_SL_OFF].p;
    if (pl.nslices > 0) {
      off[pl.nslices] += 64;
      rc = pa_spmm_pack_build((const double*)pl.a[PA_PL_VAL].p, off, (const int*)pl.a[PA_PL_SL_LEN].p, pl.nslices, 1, &pk);
      if (rc != -2 || pk.meta || pk.val || pk.pos) { printf("FAILED %s: broken offsets gave rc=%d\n", name, rc); g_failed = 1; }
    }
  }
  pa_spmm_plan_free(&pl);
  free(rowPos); free(rp); free(col); free(v);
}

int main(int argc, char** argv) {
  int fail = argc > 1 && !strcmp(argv[1], "fail-allocs");
  for (int i = 1 + fail; i < argc; ++i) one_file(argv[i], fail);
  return g_failed;
}
