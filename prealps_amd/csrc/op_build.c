/*
 * op_build.c -- the shard of one process on the host (op_build.h).  Reference behaviour kept:
 *   SymRACScaling              utils/cplm_light/cplm_matcsr.c:1461-1554
 *   ordering from a partition  utils/cplm_v0/cplm_v0_metis_utils.c:22-43,197-222
 *   symmetric permutation      utils/cplm_v0/cplm_v0_matcsr.c:941-1022
 */
#include <math.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "op_build.h"
#include "pa_alloc.h"

/* a failure: the reason into err, the shard empty again, the code to the caller through `done` */
#define OP_FAIL(code, ...) do { rc = (code); if (err && errlen) snprintf(err, errlen, __VA_ARGS__); goto done; } while (0)
#define OP_TRACE(what) do { if (in->trace) { double n_ = omp_get_wtime(); fprintf(stderr, "[setup] %-28s %.3f s\n", what, n_ - t_tr); t_tr = n_; } } while (0)

void pa_op_shard_free(pa_op_shard_t* sh) {
  free(sh->rowPos); free(sh->perm); free(sh->iperm); free(sh->d);
  free(sh->rowPtr); free(sh->colInd); free(sh->val); free(sh->src); free(sh->lcol);
  free(sh->halo_cols); free(sh->recv_by_proc);
  free(sh->peers); free(sh->send_rows); free(sh->recv_rows); free(sh->send_idx);
  memset(sh, 0, sizeof(*sh));
}

int pa_op_owner_of_part(int p, int nparts, int size) {
  /* process g owns parts [g*nparts/size, (g+1)*nparts/size) */
  int g = (int)(((long long)p * size) / nparts);
  while (g + 1 < size && (long long)(g + 1) * nparts / size <= p) ++g;
  while (g > 0 && (long long)g * nparts / size > p) --g;
  return g;
}

int pa_op_part_of_row(const int* rowPos, int nparts, int row) {
  int lo = 0, hi = nparts; /* rowPos[lo] <= row < rowPos[hi] */
  while (hi - lo > 1) {
    int mid = (lo + hi) / 2;
    if (rowPos[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

int pa_op_scaling(int N, const int* rowPtr, const double* val, int threads, double* d) {
  int zero_row = 0;
#pragma omp parallel for num_threads(threads < 1 ? 1 : threads) schedule(static) reduction(|| : zero_row)
  for (int i = 0; i < N; ++i) {
    double mx = 0.0;
    for (int k = rowPtr[i]; k < rowPtr[i + 1]; ++k) { double a = fabs(val[k]); if (a > mx) mx = a; }
    if (mx == 0.0) zero_row = 1;
    d[i] = mx > 0.0 ? sqrt(1.0 / mx) : 0.0;
  }
  return zero_row;
}

void pa_op_panel_values(int m, int row_off, const int* rowPtr, const int* colInd, const int* src, const int* perm,
                        const double* d, const double* val, int threads, double* out) {
#pragma omp parallel for num_threads(threads < 1 ? 1 : threads) schedule(static)
  for (int i = 0; i < m; ++i) {
    const int old = perm[row_off + i];
    for (int e = rowPtr[i]; e < rowPtr[i + 1]; ++e) out[e] = pa_op_panel_value(d, old, val[src[e]], perm[colInd[e]]);
  }
}

int pa_op_order(const pa_op_in_t* in, pa_op_shard_t* sh, char* err, size_t errlen) {
  int rc = PA_OP_OK;
  const int N = in->N, nparts = in->nparts, threads = in->threads < 1 ? 1 : in->threads;
  const int* rowPtr = in->rowPtr; const int* colInd = in->colInd; const int* part = in->part;
  int* fill = NULL;
  double t_tr = omp_get_wtime();
  memset(sh, 0, sizeof(*sh));
  {
    int bad_row = -1;
#pragma omp parallel for num_threads(threads) schedule(static)
    for (int i = 0; i < N; ++i) {
      int seen = 0;
      for (int k = rowPtr[i]; k < rowPtr[i + 1] && !seen; ++k) seen = colInd[k] == i;
      if (!seen) {
#pragma omp critical
        { if (bad_row < 0 || i < bad_row) bad_row = i; }
      }
    }
    if (bad_row >= 0) OP_FAIL(PA_OP_DIAG, "Diagonal is not set correctly (row %d)", bad_row);
  }
  OP_TRACE("diagonal check");
  if (in->scale) {
    sh->d = (double*)malloc((size_t)N * sizeof(double));
    if (!sh->d) OP_FAIL(PA_OP_NOMEM, "out of host memory");
    if (pa_op_scaling(N, rowPtr, in->val, threads, sh->d)) OP_FAIL(PA_OP_SCALE, "Impossible to scale the matrix, rcmin=0");
  }
  OP_TRACE("scaling");
  /* ordering: rows grouped part by part, original order inside a part */
  sh->N = N; sh->nparts = nparts;
  sh->rowPos = (int*)calloc((size_t)nparts + 1, sizeof(int));
  sh->perm = (int*)malloc((size_t)N * sizeof(int));
  sh->iperm = (int*)malloc((size_t)N * sizeof(int));
  fill = (int*)malloc((size_t)nparts * sizeof(int));
  if (!sh->rowPos || !sh->perm || !sh->iperm || !fill) OP_FAIL(PA_OP_NOMEM, "out of host memory");
  for (int i = 0; i < N; ++i) {
    int p = part ? part[i] : (int)(((long long)i * nparts) / N);
    if (p < 0 || p >= nparts) OP_FAIL(PA_OP_PART, "partition entry %d of row %d out of range", p, i);
    sh->rowPos[p + 1]++;
  }
  for (int p = 0; p < nparts; ++p) {
    if (sh->rowPos[p + 1] == 0) OP_FAIL(PA_OP_PART, "part %d is empty", p);
    sh->rowPos[p + 1] += sh->rowPos[p];
  }
  memcpy(fill, sh->rowPos, (size_t)nparts * sizeof(int));
  for (int i = 0; i < N; ++i) {
    int p = part ? part[i] : (int)(((long long)i * nparts) / N);
    sh->perm[fill[p]] = i;
    sh->iperm[i] = fill[p]++;
  }
  OP_TRACE("ordering");
done:
  free(fill);
  if (rc) pa_op_shard_free(sh);
  return rc;
}

typedef struct { int c; int k; double v; } cv_t;   /* k: where the value came from (sh->src) */
static int cmp_cv(const void* a, const void* b) {
  int ca = ((const cv_t*)a)->c, cb = ((const cv_t*)b)->c;
  return (ca > cb) - (ca < cb);
}

int pa_op_panel(const pa_op_in_t* in, pa_op_shard_t* sh, int whole, int keep_src, char* err, size_t errlen) {
  int rc = PA_OP_OK;
  const int N = sh->N, nparts = sh->nparts, rank = in->rank, size = in->size, threads = in->threads < 1 ? 1 : in->threads;
  const int* rp = in->rowPtr; const int* ci = in->colInd; const double* v = in->val;
  const int* perm = sh->perm; const int* iperm = sh->iperm; const double* d = sh->d;
  int* mark = NULL;   /* N ints: halo slot + 1 */
  double t_tr = omp_get_wtime();
  sh->part0 = (int)((long long)rank * nparts / size);
  sh->part1 = (int)((long long)(rank + 1) * nparts / size);
  sh->row_off = sh->rowPos[sh->part0];
  const int row_off = sh->row_off, m = sh->rowPos[sh->part1] - row_off;
  sh->m = m;
#define SRC(i) (whole ? perm[row_off + (i)] : (i))
  size_t lnnz = 0;
  for (int i = 0; i < m; ++i) { int r = SRC(i); lnnz += (size_t)(rp[r + 1] - rp[r]); }
  if (lnnz > 2147483000u) OP_FAIL(PA_OP_SIZE, "local panel has too many nonzeros for int32 indices");
  sh->lnnz = (int)lnnz;
  sh->rowPtr = (int*)malloc((size_t)(m + 1) * sizeof(int));
  sh->colInd = (int*)pa_big_alloc((lnnz ? lnnz : 1) * sizeof(int));
  sh->val = (double*)pa_big_alloc((lnnz ? lnnz : 1) * sizeof(double));
  if (keep_src) sh->src = (int*)pa_big_alloc((lnnz ? lnnz : 1) * sizeof(int));
  if (!sh->rowPtr || !sh->colInd || !sh->val || (keep_src && !sh->src))
    OP_FAIL(PA_OP_NOMEM, "out of host memory for the row panel (%zu entries)", lnnz);
  sh->rowPtr[0] = 0;
  {
    int maxlen = 0;
    for (int i = 0; i < m; ++i) {
      int r = SRC(i); int l = rp[r + 1] - rp[r];
      if (l > maxlen) maxlen = l;
      sh->rowPtr[i + 1] = sh->rowPtr[i] + l;
    }
    /* rows are independent: scale, renumber the columns and sort each one (threads as available) */
    int dup_row = -1;   /* (benign race: any offending row will do for the message) */
    int no_mem = 0;
    int* const colInd = sh->colInd; double* const val = sh->val; int* const src = sh->src; const int* const rowPtr = sh->rowPtr;
#pragma omp parallel num_threads(threads)
    {
      cv_t* buf = (cv_t*)malloc((maxlen ? maxlen : 1) * sizeof(cv_t));
      if (!buf) {
#pragma omp atomic write
        no_mem = 1;
      }
#pragma omp for schedule(static)
      for (int i = 0; i < m; ++i) {
        if (!buf) continue;
        int old = perm[row_off + i], r = whole ? old : i;
        int l = 0, sorted = 1;
        for (int k = rp[r]; k < rp[r + 1]; ++k, ++l) {
          buf[l].c = iperm[ci[k]];
          buf[l].k = k;
          buf[l].v = pa_op_panel_value(d, old, v[k], ci[k]);
          if (l > 0 && buf[l].c < buf[l - 1].c) sorted = 0;
        }
        if (!sorted) qsort(buf, l, sizeof(cv_t), cmp_cv);
        for (int q = 1; q < l; ++q) if (buf[q].c == buf[q - 1].c) {
#pragma omp atomic write
          dup_row = old;
        }
        int base = rowPtr[i];
        for (int q = 0; q < l; ++q) { colInd[base + q] = buf[q].c; val[base + q] = buf[q].v; }
        if (src) for (int q = 0; q < l; ++q) src[base + q] = buf[q].k;
      }
      free(buf);
    }
    if (no_mem) OP_FAIL(PA_OP_NOMEM, "out of host memory");
    if (dup_row >= 0)
      OP_FAIL(PA_OP_DUP, "row %d holds the same column twice: sum duplicate entries before building the operator", dup_row);
  }
#undef SRC
  OP_TRACE("permute + sort rows");
  /* halo: off-process columns, grouped by owner (ascending global index) */
  const int lo = row_off, hi = row_off + m;
  mark = (int*)calloc((size_t)N, sizeof(int));
  if (!mark) OP_FAIL(PA_OP_NOMEM, "out of host memory");
  int halo = 0;
  for (size_t k = 0; k < lnnz; ++k) { int c = sh->colInd[k]; if ((c < lo || c >= hi) && !mark[c]) { mark[c] = 1; ++halo; } }
  sh->halo_cols = (int*)malloc((halo ? halo : 1) * sizeof(int));
  sh->recv_by_proc = (int*)calloc((size_t)(size > 0 ? size : 1), sizeof(int));
  sh->lcol = (int*)pa_big_alloc((lnnz + 8) * sizeof(int));
  if (!sh->halo_cols || !sh->recv_by_proc || !sh->lcol) OP_FAIL(PA_OP_NOMEM, "out of host memory");
  { int q = 0; for (int c = 0; c < N; ++c) if (mark[c]) { sh->halo_cols[q] = c; mark[c] = ++q; } }
  sh->halo = halo;
  OP_TRACE("halo marks");
  for (int q = 0; q < halo; ++q)
    sh->recv_by_proc[pa_op_owner_of_part(pa_op_part_of_row(sh->rowPos, nparts, sh->halo_cols[q]), nparts, size)]++;
  /* local column ids */
  {
    const int* const colInd = sh->colInd; int* const lcol = sh->lcol;
#pragma omp parallel for num_threads(threads) schedule(static)
    for (long long k = 0; k < (long long)lnnz; ++k) { int c = colInd[k]; lcol[k] = (c >= lo && c < hi) ? c - lo : m + mark[c] - 1; }
    for (size_t k = lnnz; k < lnnz + 8; ++k) lcol[k] = 0;
  }
  OP_TRACE("local columns");
done:
  free(mark);
  if (rc) pa_op_shard_free(sh);
  return rc;
}

int pa_op_finish_peers(pa_op_shard_t* sh, int size, int* asked, const int* asked_cnt, char* err, size_t errlen) {
  int rc = PA_OP_OK;
  const size_t room = (size_t)(size > 0 ? size : 1);
  sh->peers = (int*)malloc(room * sizeof(int));
  sh->send_rows = (int*)calloc(room, sizeof(int));
  sh->recv_rows = (int*)calloc(room, sizeof(int));
  if (!sh->peers || !sh->send_rows || !sh->recv_rows) OP_FAIL(PA_OP_NOMEM, "out of host memory");
  sh->nsend = 0; sh->npeers = 0;
  for (int g = 0; g < size; ++g) {
    if (asked_cnt[g] || sh->recv_by_proc[g]) {
      sh->peers[sh->npeers] = g; sh->recv_rows[sh->npeers] = sh->recv_by_proc[g]; sh->send_rows[sh->npeers] = asked_cnt[g];
      sh->npeers++;
    }
    sh->nsend += asked_cnt[g];
  }
  sh->send_idx = asked; asked = NULL;
done:
  free(asked);
  if (rc) pa_op_shard_free(sh);
  return rc;
}

int pa_op_peers_whole(const pa_op_in_t* in, pa_op_shard_t* sh, char* err, size_t errlen) {
  int rc = PA_OP_OK;
  const int N = sh->N, nparts = sh->nparts, rank = in->rank, size = in->size, threads = in->threads < 1 ? 1 : in->threads;
  const int m = sh->m, lo = sh->row_off, hi = sh->row_off + m;
  const int* rowPtr = in->rowPtr; const int* colInd = in->colInd; const int* iperm = sh->iperm; const int* rowPos = sh->rowPos;
  unsigned char* need = NULL;   /* need[g * m + i]: process g reads our local row i */
  int* send_idx = NULL; int* asked_cnt = NULL;
  double t_tr = omp_get_wtime();
  /* Every process holds the whole matrix here, so this needs no communication and, unlike taking "our rows
   * that touch a column of g", it stays right for a pattern that is not structurally symmetric (a `general`
   * .mtx with explicit zeros dropped on one side). */
  if (size > 1) {
    need = (unsigned char*)calloc((size_t)size * (m ? m : 1), 1);
    if (!need) OP_FAIL(PA_OP_NOMEM, "out of host memory for the halo plan");
#pragma omp parallel for num_threads(threads) schedule(dynamic, 4096)
    for (int i = 0; i < N; ++i) {
      int r = iperm[i];
      if (r >= lo && r < hi) continue;
      unsigned char* ng = need + (size_t)pa_op_owner_of_part(pa_op_part_of_row(rowPos, nparts, r), nparts, size) * m;
      for (int k = rowPtr[i]; k < rowPtr[i + 1]; ++k) {
        int c = iperm[colInd[k]];
        if (c >= lo && c < hi) ng[c - lo] = 1;   /* (all writers store the same value) */
      }
    }
  }
  asked_cnt = (int*)calloc((size_t)(size > 0 ? size : 1), sizeof(int));
  if (!asked_cnt) OP_FAIL(PA_OP_NOMEM, "out of host memory for the halo plan");
  size_t nsend = 0;
  for (int g = 0; need && g < size; ++g) {
    if (g == rank) continue;
    for (int i = 0; i < m; ++i) asked_cnt[g] += need[(size_t)g * m + i];
    nsend += (size_t)asked_cnt[g];
  }
  send_idx = (int*)malloc((nsend ? nsend : 1) * sizeof(int));
  if (!send_idx) OP_FAIL(PA_OP_NOMEM, "out of host memory for the halo plan");
  nsend = 0;
  for (int g = 0; need && g < size; ++g) {
    if (g == rank) continue;
    for (int i = 0; i < m; ++i) if (need[(size_t)g * m + i]) send_idx[nsend++] = i;
  }
  rc = pa_op_finish_peers(sh, size, send_idx, asked_cnt, err, errlen);
  send_idx = NULL;   /* (taken over) */
  OP_TRACE("peer lists");
done:
  free(need); free(send_idx); free(asked_cnt);
  if (rc) pa_op_shard_free(sh);
  return rc;
}

void pa_op_inverse_send_list(int m, int nsend, const int* send_idx, int* off, int* slot) {
  for (int i = 0; i < nsend; ++i) ++off[send_idx[i] + 2];
  for (int r = 0; r < m; ++r) off[r + 2] += off[r + 1];       /* off[r + 1] = first slot entry of row r */
  for (int i = 0; i < nsend; ++i) slot[off[send_idx[i] + 1]++] = i;   /* ... now off[r + 1] = end of row r */
}
