/*
 * bj_build_check.c -- runs the host unit of the block-Jacobi create (prealps_amd/csrc/bj_build.c) on cases that
 * tests/test_bj_build_cpu.py writes, and dumps every array it produces for the test to compare.  No judgement
 * here beyond the sanitizers the test builds it with: usage  bj_build_check <cases in> <arrays out>.
 *
 * Cases file (native binary), case after case, each beginning with an int32 kind:
 *   1 blocks: int32 np, m, nnz, row_off, nd_mode, nd_rows, dev_factor, dev_wmax, threads, wide_from;
 *             int32 grow[np + 1], rowPtr[m + 1], colInd[nnz]; float64 val[nnz]
 *             -> pa_bj_build_blocks; for a host-factored build also pa_bj_layout_slab over every block
 *   2 layout: int32 np, factor_wmax, max_R, g4_max_band, g4_max_rows, dev_factor, wide_from, want_g4, want_pairs;
 *             int32 nrows[np], bw[np], is_nd[np]                   -> pa_bj_layout_build
 *   3 cholesky: int32 b, w; float64 band[b * (w + 1)]              -> pa_bj_band_cholesky
 * Arrays file: records of  char name[32] ("<case>.<field>"), char type ('i' int32, 'q' int64, 'd' float64, 'c' text),
 * int64 count, then the values.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_build.h"

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
  const size_t size = type == 'i' ? 4 : (type == 'c' ? 1 : 8);
  memset(name, 0, sizeof(name));
  snprintf(name, sizeof(name), "%d.%s", g_case, field);
  fwrite(name, 1, sizeof(name), g_out); fwrite(&type, 1, 1, g_out); fwrite(&cnt, sizeof(cnt), 1, g_out);
  if (n) fwrite(p, size, n, g_out);
}
static void put_int(const char* field, long long v) { int64_t x = v; put(field, 'q', &x, 1); }
static void put_blk(const char* field, int q, char type, const void* p, size_t n) {
  char f[24];
  snprintf(f, sizeof(f), "%s%d", field, q);
  put(f, type, p, n);
}

static void case_blocks(void) {
  int h[10];
  get(h, sizeof(int), 10);
  const int np = h[0], m = h[1], nnz = h[2], wide_from = h[9];
  int* grow = get_ints((size_t)np + 1);
  int* rp = get_ints((size_t)m + 1);
  int* ci = get_ints((size_t)nnz);
  double* v = must(malloc(((size_t)nnz + 1) * sizeof(double)));
  get(v, sizeof(double), (size_t)nnz);
  const pa_bj_build_in_t in = {.np = np, .m = m, .rowPtr = rp, .colInd = ci, .val = v, .grow = grow, .row_off = h[3],
                               .nd_mode = h[4], .nd_rows = h[5], .dev_factor = h[6], .dev_wmax = h[7], .threads = h[8]};
  pa_bj_build_t B;
  const int rc = pa_bj_build_blocks(&in, &B);
  put_int("rc", rc); put_int("fail_row", B.fail_row); put_int("nomem_block", B.nomem_block);
  if (rc) {     /* what a failed build leaves: nothing */
    put_int("empty", !B.row0 && !B.nrows && !B.bw && !B.is_nd && !B.map_f && !B.map_b && !B.invd_f && !B.invd_b && !B.bands &&
                     !B.coo_off && !B.coo_val && !B.coo_n && B.np == 0);
  } else {
    put("row0", 'i', B.row0, (size_t)np); put("nrows", 'i', B.nrows, (size_t)np); put("bw", 'i', B.bw, (size_t)np);
    put("is_nd", 'c', B.is_nd, (size_t)np);
    put("map_f", 'i', B.map_f, (size_t)m); put("map_b", 'i', B.map_b, (size_t)m);
    for (int q = 0; q < np; ++q) {
      const size_t b = (size_t)B.nrows[q], w = (size_t)B.bw[q];
      if (B.bands[q]) put_blk("band", q, 'd', B.bands[q], b * (w + 1));
      if (B.coo_off[q]) { put_blk("coo_off", q, 'q', B.coo_off[q], B.coo_n[q]); put_blk("coo_val", q, 'd', B.coo_val[q], B.coo_n[q]); }
    }
    if (!in.dev_factor) {     /* the sweep records of the host-factored blocks, slab by slab */
      for (int q = 0; q < np; ++q) {
        if (B.is_nd[q]) continue;
        const size_t len = (size_t)B.nrows[q] * (size_t)pa_bj_reclen(B.bw[q], wide_from);
        double* f = must(calloc(len ? len : 1, sizeof(double)));
        double* g = must(calloc(len ? len : 1, sizeof(double)));
        for (int j0 = 0; j0 < B.nrows[q]; j0 += 256) pa_bj_layout_slab(&B, wide_from, q, j0, f, g);
        put_blk("Lf", q, 'd', f, len); put_blk("Lb", q, 'd', g, len);
        free(f); free(g);
      }
      put("invd_f", 'd', B.invd_f, (size_t)m); put("invd_b", 'd', B.invd_b, (size_t)m);
    }
  }
  pa_bj_build_free(&B);
  pa_bj_build_free(&B);     /* (a second release of an empty build is harmless) */
  free(grow); free(rp); free(ci); free(v);
}

static void case_layout(void) {
  int h[9];
  get(h, sizeof(int), 9);
  const int np = h[0];
  int* nrows = get_ints((size_t)np);
  int* bw = get_ints((size_t)np);
  int* nd = get_ints((size_t)np);
  char* is_nd = must(malloc((size_t)np + 1));
  for (int q = 0; q < np; ++q) is_nd[q] = (char)nd[q];
  const pa_bj_layout_in_t in = {.np = np, .nrows = nrows, .bw = bw, .is_nd = is_nd, .factor_wmax = h[1], .max_R = h[2],
                                .g4_max_band = h[3], .g4_max_rows = h[4], .dev_factor = h[5], .wide_from = h[6],
                                .want_g4 = h[7], .want_pairs = h[8]};
  pa_bj_layout_t L;
  char err[256];
  memset(err, 'x', sizeof(err));
  const int rc = pa_bj_layout_build(&in, &L, err, sizeof(err));
  put_int("rc", rc); put_int("bad_bw", L.bad_bw);
  put("err", 'c', err, strlen(err));
  if (rc) {
    const int bad_bw = L.bad_bw;
    pa_bj_layout_t Z;
    memset(&Z, 0, sizeof(Z));
    L.bad_bw = 0;
    put_int("empty", !memcmp(&L, &Z, sizeof(Z)));
    L.bad_bw = bad_bw;
  } else {
    const size_t n1 = (size_t)np + 1;
    put_int("wide_from", L.wide_from); put_int("tot", (long long)L.tot); put_int("maxrec", L.maxrec); put_int("pad", (long long)L.pad);
    put_int("ndev", L.ndev); put_int("nnd", L.nnd); put_int("max_bw", L.max_bw); put_int("nclass", L.nclass);
    put_int("any_g4", L.any_g4); put_int("any_pairs", L.any_pairs); put_int("tot2", L.tot2); put_int("btot", (long long)L.btot);
    put_int("ns", L.ns); put_int("wsmall", L.wsmall); put_int("nbig", L.nbig); put_int("wbig", L.wbig);
    put("off", 'q', L.off, n1); put("off2", 'q', L.off2, n1); put("boff", 'q', L.boff, n1);
    put("slist", 'i', L.slist, (size_t)L.ns); put("blist", 'i', L.blist, (size_t)L.nbig);
    put("class_R", 'i', L.class_R, (size_t)L.nclass); put("class_count", 'i', L.class_count, (size_t)L.nclass);
    put("class_wmax", 'i', L.class_wmax, (size_t)L.nclass); put("class_bmax", 'i', L.class_bmax, (size_t)L.nclass);
    put("class_g4", 'i', L.class_g4, (size_t)L.nclass); put("class_pairs", 'i', L.class_pairs, (size_t)L.nclass);
    for (int c = 0; c < L.nclass; ++c) put_blk("class_list", c, 'i', L.class_list[c], (size_t)L.class_count[c]);
  }
  pa_bj_layout_free(&L);
  pa_bj_layout_free(&L);
  free(nrows); free(bw); free(nd); free(is_nd);
}

static void case_cholesky(void) {
  int h[2];
  get(h, sizeof(int), 2);
  const size_t len = (size_t)h[0] * ((size_t)h[1] + 1);
  double* band = must(malloc((len ? len : 1) * sizeof(double)));
  get(band, sizeof(double), len);
  put_int("bad", pa_bj_band_cholesky(band, h[0], h[1]));
  put("band", 'd', band, len);
  free(band);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <cases in> <arrays out>\n", argv[0]); return 2; }
  g_in = fopen(argv[1], "rb");
  g_out = fopen(argv[2], "wb");
  if (!g_in || !g_out) { fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]); return 2; }
  int kind;
  for (g_case = 0; fread(&kind, sizeof(int), 1, g_in) == 1; ++g_case) {
    if (kind == 1) case_blocks();
    else if (kind == 2) case_layout();
    else if (kind == 3) case_cholesky();
    else { fprintf(stderr, "case %d: unknown kind %d\n", g_case, kind); return 2; }
  }
  fclose(g_in);
  if (fclose(g_out)) { fprintf(stderr, "writing %s failed\n", argv[2]); return 2; }
  return 0;
}
