/* Stand-alone run of prealps_amd/csrc/op_build.c (tests/test_op_build_cpu.py).  usage: op_build_check <case file>
 * The file: "N nnz size nparts have_part scale keep_src threads", then rowPtr (N + 1), colInd, val (nnz each) and,
 * with have_part, N part ids.  For every rank of `size` the shard is built as the replicated build does (order,
 * panel from the whole matrix, send lists from the whole matrix) and printed, one array per line as
 * "name count values..."; a failed build prints "error <code> <message>" and "empty <0|1>" (1: the shard came back as
 * pa_op_shard_free leaves it).  Two more lines per rank: "whole0 <0|1>" -- with size > 1, the panel built with
 * whole = 0 from this rank's raw rows alone equals the one above, array for array -- and "values <0|1>" -- with
 * keep_src, pa_op_panel_values through src reproduces the panel's values in bits. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "op_build.h"

static void ints(const char* name, const int* a, long long n) {
  printf("%s %lld", name, n);
  for (long long i = 0; i < n; ++i) printf(" %d", a[i]);
  printf("\n");
}
static void doubles(const char* name, const double* a, long long n) {
  printf("%s %lld", name, n);
  for (long long i = 0; i < n; ++i) printf(" %.17g", a[i]);
  printf("\n");
}
static void* xmalloc(size_t bytes) {
  void* p = malloc(bytes ? bytes : 1);
  if (!p) { printf("out of memory in the check itself\n"); exit(3); }
  return p;
}
static void* copy_of(const void* p, size_t bytes) { return memcpy(xmalloc(bytes), p, bytes); }
static int same(const void* a, const void* b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }
static int is_empty(const pa_op_shard_t* sh) {
  pa_op_shard_t zero;
  memset(&zero, 0, sizeof(zero));
  return memcmp(sh, &zero, sizeof(zero)) == 0;
}
static void failed(int rc, const char* err, const pa_op_shard_t* sh) {
  printf("error %d %s\nempty %d\n", rc, err, is_empty(sh));
}

/* the panel of in->rank from its raw rows alone, on a copy of the ordering: what a rank that was sent its rows does */
static int whole0_agrees(const pa_op_in_t* in, const pa_op_shard_t* sh, int keep_src) {
  const int m = sh->m;
  int* lrp = (int*)xmalloc(((size_t)m + 1) * sizeof(int));
  int* lci = (int*)xmalloc((size_t)sh->lnnz * sizeof(int));
  double* lv = (double*)xmalloc((size_t)sh->lnnz * sizeof(double));
  lrp[0] = 0;
  for (int i = 0; i < m; ++i) {
    const int old = sh->perm[sh->row_off + i], l = in->rowPtr[old + 1] - in->rowPtr[old];
    memcpy(lci + lrp[i], in->colInd + in->rowPtr[old], (size_t)l * sizeof(int));
    memcpy(lv + lrp[i], in->val + in->rowPtr[old], (size_t)l * sizeof(double));
    lrp[i + 1] = lrp[i] + l;
  }
  pa_op_shard_t s2;
  memset(&s2, 0, sizeof(s2));
  s2.N = sh->N; s2.nparts = sh->nparts;
  s2.rowPos = (int*)copy_of(sh->rowPos, ((size_t)sh->nparts + 1) * sizeof(int));
  s2.perm = (int*)copy_of(sh->perm, (size_t)sh->N * sizeof(int));
  s2.iperm = (int*)copy_of(sh->iperm, (size_t)sh->N * sizeof(int));
  if (sh->d) s2.d = (double*)copy_of(sh->d, (size_t)sh->N * sizeof(double));
  pa_op_in_t in2 = *in;
  in2.rowPtr = lrp; in2.colInd = lci; in2.val = lv; in2.part = NULL;
  char err[256];
  int ok = pa_op_panel(&in2, &s2, 0, keep_src, err, sizeof(err)) == PA_OP_OK;
  const size_t nz = (size_t)sh->lnnz;
  ok = ok && s2.part0 == sh->part0 && s2.part1 == sh->part1 && s2.row_off == sh->row_off && s2.m == m &&
       s2.lnnz == sh->lnnz && s2.halo == sh->halo && same(s2.rowPtr, sh->rowPtr, ((size_t)m + 1) * sizeof(int)) &&
       same(s2.colInd, sh->colInd, nz * sizeof(int)) && same(s2.val, sh->val, nz * sizeof(double)) &&
       same(s2.lcol, sh->lcol, (nz + 8) * sizeof(int)) && same(s2.halo_cols, sh->halo_cols, (size_t)sh->halo * sizeof(int)) &&
       same(s2.recv_by_proc, sh->recv_by_proc, (size_t)in->size * sizeof(int)) && (s2.src != NULL) == (sh->src != NULL);
  if (ok && keep_src)   /* the same entry of the same row: one index counts from the raw rows, the other from the whole matrix */
    for (int i = 0; i < m; ++i)
      for (int e = sh->rowPtr[i]; e < sh->rowPtr[i + 1]; ++e)
        ok = ok && s2.src[e] - lrp[i] == sh->src[e] - in->rowPtr[sh->perm[sh->row_off + i]];
  pa_op_shard_free(&s2);
  free(lrp); free(lci); free(lv);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int N, nnz, size, nparts, have_part, scale, keep_src, threads, okr = 1;
  if (fscanf(f, "%d %d %d %d %d %d %d %d", &N, &nnz, &size, &nparts, &have_part, &scale, &keep_src, &threads) != 8) return 2;
  int* rp = (int*)xmalloc(((size_t)N + 1) * sizeof(int));
  int* ci = (int*)xmalloc((size_t)nnz * sizeof(int));
  double* v = (double*)xmalloc((size_t)nnz * sizeof(double));
  int* part = have_part ? (int*)xmalloc((size_t)N * sizeof(int)) : NULL;
  for (int i = 0; i <= N; ++i) okr = okr && fscanf(f, "%d", &rp[i]) == 1;
  for (int k = 0; k < nnz; ++k) okr = okr && fscanf(f, "%d", &ci[k]) == 1;
  for (int k = 0; k < nnz; ++k) okr = okr && fscanf(f, "%lf", &v[k]) == 1;
  for (int i = 0; part && i < N; ++i) okr = okr && fscanf(f, "%d", &part[i]) == 1;
  fclose(f);
  if (!okr) { fprintf(stderr, "short case file\n"); return 2; }
  for (int rank = 0; rank < size; ++rank) {
    const pa_op_in_t in = {.N = N, .rowPtr = rp, .colInd = ci, .val = v, .nparts = nparts, .part = part, .scale = scale,
                           .rank = rank, .size = size, .threads = threads, .trace = 0};
    pa_op_shard_t sh;
    char err[256] = "";
    memset(&sh, 0x5a, sizeof(sh));   /* (pa_op_order zeroes it) */
    printf("rank %d\n", rank);
    int rc = pa_op_order(&in, &sh, err, sizeof(err));
    if (rc) { failed(rc, err, &sh); continue; }
    rc = pa_op_panel(&in, &sh, 1, keep_src, err, sizeof(err));
    if (rc) { failed(rc, err, &sh); continue; }
    rc = pa_op_peers_whole(&in, &sh, err, sizeof(err));
    if (rc) { failed(rc, err, &sh); continue; }
    const int head[10] = {sh.N, sh.nparts, sh.part0, sh.part1, sh.row_off, sh.m, sh.lnnz, sh.halo, sh.npeers, sh.nsend};
    ints("head", head, 10);
    ints("rowPos", sh.rowPos, (long long)nparts + 1);
    ints("perm", sh.perm, N);
    ints("iperm", sh.iperm, N);
    doubles("d", sh.d, sh.d ? N : 0);
    ints("rowPtr", sh.rowPtr, (long long)sh.m + 1);
    ints("colInd", sh.colInd, sh.lnnz);
    doubles("val", sh.val, sh.lnnz);
    ints("src", sh.src, sh.src ? sh.lnnz : 0);
    ints("lcol", sh.lcol, (long long)sh.lnnz + 8);
    ints("halo_cols", sh.halo_cols, sh.halo);
    ints("recv_by_proc", sh.recv_by_proc, size);
    ints("peers", sh.peers, sh.npeers);
    ints("send_rows", sh.send_rows, sh.npeers);
    ints("recv_rows", sh.recv_rows, sh.npeers);
    ints("send_idx", sh.send_idx, sh.nsend);
    {
      int* off = (int*)xmalloc(((size_t)sh.m + 2) * sizeof(int));
      int* slot = (int*)xmalloc((size_t)sh.nsend * sizeof(int));
      memset(off, 0, ((size_t)sh.m + 2) * sizeof(int));
      pa_op_inverse_send_list(sh.m, sh.nsend, sh.send_idx, off, slot);
      ints("pk_off", off, (long long)sh.m + 1);
      ints("pk_slot", slot, sh.nsend);
      free(off); free(slot);
    }
    printf("whole0 %d\n", size > 1 ? whole0_agrees(&in, &sh, keep_src) : 1);
    if (keep_src) {
      double* again = (double*)xmalloc((size_t)sh.lnnz * sizeof(double));
      pa_op_panel_values(sh.m, sh.row_off, sh.rowPtr, sh.colInd, sh.src, sh.perm, sh.d, v, threads, again);
      printf("values %d\n", same(again, sh.val, (size_t)sh.lnnz * sizeof(double)));
      free(again);
    } else printf("values 1\n");
    pa_op_shard_free(&sh);
    if (!is_empty(&sh)) { fprintf(stderr, "pa_op_shard_free left something behind\n"); return 1; }
  }
  free(rp); free(ci); free(v); free(part);
  return 0;
}
