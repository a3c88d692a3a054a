/*
 * coarse_space.c -- the coarse space of the two-level block-Jacobi preconditioner, host side (coarse_space.h).
 * libc + OpenMP only.  Every sum has one fixed order: the results are the same bits for any number of threads.
 */
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "coarse_space.h"

static int cs_fail(int code, char* err, size_t errlen, const char* fmt, ...) {
  if (err && errlen) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, errlen, fmt, ap);
    va_end(ap);
  }
  return code;
}

void pa_coarse_free(pa_coarse_t* c) {
  if (!c) return;
  free(c->zv); free(c->ch_row0); free(c->ch_nrows); free(c->ch_aggr); free(c->agg_ptr); free(c->agg_chunk);
  free(c->E); free(c->Einv); free(c->rows);
  memset(c, 0, sizeof(*c));
}

/* ---- chunk lists ---------------------------------------------------------------------------------- */
static int cs_chunks(const pa_coarse_share_in_t* in, pa_coarse_t* c) {
  const int p0 = in->part0, p1 = in->part0 + in->np_loc, off = in->row_off, CH = PA_COARSE_CHUNK;
  int nch = 0;
  for (int p = p0; p < p1; ++p) nch += (in->rowPos[p + 1] - in->rowPos[p] + CH - 1) / CH;
  c->nchunks = nch;
  c->ch_row0 = (int*)malloc((size_t)(nch ? nch : 1) * sizeof(int));
  c->ch_nrows = (int*)malloc((size_t)(nch ? nch : 1) * sizeof(int));
  c->ch_aggr = (int*)malloc((size_t)(nch ? nch : 1) * sizeof(int));
  c->agg_ptr = (int*)calloc((size_t)c->naggr + 1, sizeof(int));
  c->agg_chunk = (int*)malloc((size_t)(nch ? nch : 1) * sizeof(int));
  if (!c->ch_row0 || !c->ch_nrows || !c->ch_aggr || !c->agg_ptr || !c->agg_chunk) return PA_COARSE_NOMEM;
  nch = 0;
  for (int p = p0; p < p1; ++p)
    for (int r = in->rowPos[p]; r < in->rowPos[p + 1]; r += CH) {
      const int left = in->rowPos[p + 1] - r;
      c->ch_row0[nch] = r - off; c->ch_nrows[nch] = left < CH ? left : CH; c->ch_aggr[nch] = in->part_aggregate[p];
      c->agg_ptr[in->part_aggregate[p] + 1]++;
      ++nch;
    }
  for (int g = 0; g < c->naggr; ++g) c->agg_ptr[g + 1] += c->agg_ptr[g];
  int* fill = (int*)malloc((size_t)(c->naggr ? c->naggr : 1) * sizeof(int));
  if (!fill) return PA_COARSE_NOMEM;
  for (int g = 0; g < c->naggr; ++g) fill[g] = c->agg_ptr[g];
  for (int x = 0; x < nch; ++x) c->agg_chunk[fill[c->ch_aggr[x]]++] = x;      /* ascending inside an aggregate */
  free(fill);
  /* the coarse rows this share needs: those of the aggregates with a chunk here, ascending */
  int need = 0;
  for (int g = 0; g < c->naggr; ++g) need += c->agg_ptr[g + 1] > c->agg_ptr[g];
  c->nrows = need * c->k;
  c->rows = (int*)malloc((size_t)(c->nrows ? c->nrows : 1) * sizeof(int));
  if (!c->rows) return PA_COARSE_NOMEM;
  need = 0;
  for (int g = 0; g < c->naggr; ++g)
    if (c->agg_ptr[g + 1] > c->agg_ptr[g])
      for (int a = 0; a < c->k; ++a) c->rows[need++] = g * c->k + a;
  return PA_COARSE_OK;
}

/* ---- E = Z^T A Z ---------------------------------------------------------------------------------- */
/* the part of global row j (0 <= j < rowPos[np]): the last p with rowPos[p] <= j, which skips parts without rows */
static inline int cs_part_of(const int* rowPos, int np, int j) {
  int lo = 0, hi = np;                     /* rowPos[lo] <= j < rowPos[hi] */
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (rowPos[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

/* The share's rows of E: the sum over the local rows i alone; column j (global) goes to the aggregate of its part. */
static int cs_assemble(const pa_coarse_share_in_t* in, pa_coarse_t* c, int threads) {
  const int m = in->m, k = c->k, nc = c->nc, off = in->row_off, np = in->nparts, N = in->rowPos[np];
  int* row_aggr = (int*)malloc((size_t)(m ? m : 1) * sizeof(int));
  if (!row_aggr) return PA_COARSE_NOMEM;
  for (int x = 0; x < c->nchunks; ++x)
    for (int i = c->ch_row0[x]; i < c->ch_row0[x] + c->ch_nrows[x]; ++i) row_aggr[i] = c->ch_aggr[x];
  const double* zv = c->zv;
  const double* Vp = in->Vp;
  double* E = c->E;
  /* aggregate g owns the rows g*k .. g*k + k - 1 of E: its chunks in list order, their rows and entries in order */
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1)
  for (int g = 0; g < c->naggr; ++g) {
    double* Eg = E + (size_t)g * k * nc;
    for (int x = c->agg_ptr[g]; x < c->agg_ptr[g + 1]; ++x) {
      const int ch = c->agg_chunk[x];
      for (int i = c->ch_row0[ch]; i < c->ch_row0[ch] + c->ch_nrows[ch]; ++i) {
        const double* zi = zv + (size_t)i * k;
        for (int e = in->rowPtr[i]; e < in->rowPtr[i + 1]; ++e) {
          const int j = in->gcol[e];
          if (j < 0 || j >= N) continue;
          const double* zj = Vp + (size_t)j * k;
          const double aij = in->val[e];
          const int h = j >= off && j - off < m ? row_aggr[j - off] : in->part_aggregate[cs_part_of(in->rowPos, np, j)];
          double* Eh = Eg + (size_t)h * k;
          for (int a = 0; a < k; ++a) {
            const double za = zi[a] * aij;
            for (int b = 0; b < k; ++b) Eh[(size_t)a * nc + b] += za * zj[b];
          }
        }
      }
    }
  }
  free(row_aggr);
  return PA_COARSE_OK;
}

/* ---- Einv = L^-T L^-1 ------------------------------------------------------------------------------ */
/* dot product in one fixed order: four running sums over i mod 4, folded at the end */
static inline double cs_dot(const double* x, const double* y, int n) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int i = 0;
  for (; i + 4 <= n; i += 4) { s0 += x[i] * y[i]; s1 += x[i + 1] * y[i + 1]; s2 += x[i + 2] * y[i + 2]; s3 += x[i + 3] * y[i + 3]; }
  for (; i < n; ++i) s0 += x[i] * y[i];
  return (s0 + s1) + (s2 + s3);
}

static int cs_invert(pa_coarse_t* c, int threads, char* err, size_t errlen) {
  c->bad_aggr = c->bad_vec = -1;
  const int n = c->nc, k = c->k;
  const size_t nn = (size_t)n * n;
  double* L = (double*)malloc((nn ? nn : 1) * sizeof(double));
  double* X = (double*)calloc(nn ? nn : 1, sizeof(double));
  if (!L || !X) { free(L); free(X); return cs_fail(PA_COARSE_NOMEM, err, errlen, "out of host memory for the %d x %d coarse matrix", n, n); }
  memcpy(L, c->E, nn * sizeof(double));
  double maxd = 0.0;
  for (int j = 0; j < n; ++j) { const double d = L[(size_t)j * n + j]; if (d > maxd) maxd = d; }
  const double floor_ = (double)n * DBL_EPSILON * maxd;
  /* Cholesky-Crout on the lower triangle, row major: column j at a time, its rows shared among the threads */
  int bad = -1;
  double badp = 0.0;
  for (int j = 0; j < n && bad < 0; ++j) {
    double* Lj = L + (size_t)j * n;
    const double d = Lj[j] - cs_dot(Lj, Lj, j);
    if (!(d > floor_)) { bad = j; badp = d; break; }
    const double ljj = sqrt(d), inv = 1.0 / ljj;
    Lj[j] = ljj;
#pragma omp parallel for num_threads(threads) schedule(static) if (n - j > 128)
    for (int i = j + 1; i < n; ++i) {
      double* Li = L + (size_t)i * n;
      Li[j] = (Li[j] - cs_dot(Li, Lj, j)) * inv;
    }
  }
  if (bad >= 0) {
    c->bad_aggr = bad / k; c->bad_vec = bad % k;
    free(L); free(X);
    return cs_fail(PA_COARSE_SINGULAR, err, errlen,
                   "the coarse matrix E = Z^T A Z is singular: pivot %.3e <= %.3e at aggregate %d, vector %d (the vectors "
                   "are linearly dependent on that aggregate, or vanish there)", badp, floor_, bad / k, bad % k);
  }
  /* X = L^-1 (lower): a thread owns blocks of columns and runs every row for them */
  const int CB = 32;
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1)
  for (int j0 = 0; j0 < n; j0 += CB) {
    const int j1 = j0 + CB < n ? j0 + CB : n;
    for (int i = j0; i < n; ++i) {
      const double* Li = L + (size_t)i * n;
      double* Xi = X + (size_t)i * n;
      const int je = i + 1 < j1 ? i + 1 : j1;            /* columns j0 .. je - 1 of row i are inside the triangle */
      for (int j = j0; j < je; ++j) Xi[j] = (i == j) ? 1.0 : 0.0;
      for (int q = j0; q < i; ++q) {                      /* X(i, j) -= L(i, q) X(q, j), j <= q */
        const double l = Li[q];
        const double* Xq = X + (size_t)q * n;
        const int jq = q + 1 < je ? q + 1 : je;
        for (int j = j0; j < jq; ++j) Xi[j] -= l * Xq[j];
      }
      const double inv = 1.0 / Li[i];
      for (int j = j0; j < je; ++j) Xi[j] *= inv;
    }
  }
  /* Einv(i, j) = sum_{q >= i} X(q, i) X(q, j) for j <= i, then the mirror */
  double* Ei = c->Einv;
  memset(Ei, 0, nn * sizeof(double));
#pragma omp parallel for num_threads(threads) schedule(dynamic, 8)
  for (int i = 0; i < n; ++i) {
    double* row = Ei + (size_t)i * n;
    for (int q = i; q < n; ++q) {
      const double* Xq = X + (size_t)q * n;
      const double xi = Xq[i];
      for (int j = 0; j <= i; ++j) row[j] += xi * Xq[j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j) Ei[(size_t)j * n + i] = Ei[(size_t)i * n + j];
  free(L); free(X);
  return PA_COARSE_OK;
}

static int cs_threads(int want) {
  if (want > 0) return want;
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}

/* ---- stage (a): a rank's share ---------------------------------------------------------------------- */
int pa_coarse_share(const pa_coarse_share_in_t* in, pa_coarse_t* c, char* err, size_t errlen) {
  if (!c) return PA_COARSE_ARG;
  memset(c, 0, sizeof(*c));
  c->bad_aggr = c->bad_vec = -1;
  if (!in || in->m < 0 || in->nparts < 1 || !in->rowPtr || !in->gcol || !in->val || !in->rowPos || !in->part_aggregate || !in->Vp)
    return cs_fail(PA_COARSE_ARG, err, errlen, "invalid arguments");
  if (in->row_off < 0 || in->part0 < 0 || in->np_loc < 0 || in->part0 + in->np_loc > in->nparts ||
      in->rowPos[in->part0] != in->row_off || in->rowPos[in->part0 + in->np_loc] != in->row_off + in->m)
    return cs_fail(PA_COARSE_ARG, err, errlen, "the %d rows from row %d are not the parts %d .. %d", in->m, in->row_off,
                   in->part0, in->part0 + in->np_loc - 1);
  if (in->k < 1 || in->k > PA_COARSE_MAX_VECS)
    return cs_fail(PA_COARSE_ARG, err, errlen, "k = %d vectors: expected 1 .. %d", in->k, PA_COARSE_MAX_VECS);
  const int cap = in->max_dofs > 0 ? in->max_dofs : PA_COARSE_MAX_DOFS;
  if (in->naggr < 1 || (long long)in->naggr * in->k > cap)
    return cs_fail(PA_COARSE_CAP, err, errlen, "%d aggregates x %d vectors = %lld coarse unknowns, the cap is %d",
                   in->naggr, in->k, (long long)in->naggr * in->k, cap);
  const int m = in->m, k = in->k, naggr = in->naggr, threads = cs_threads(in->threads);
  /* every aggregate in range and non-empty (a part without rows holds nothing), over the parts of all shares */
  {
    int* cnt = (int*)calloc((size_t)naggr, sizeof(int));
    if (!cnt) return cs_fail(PA_COARSE_NOMEM, err, errlen, "out of host memory");
    for (int p = 0; p < in->nparts; ++p) {
      const int g = in->part_aggregate[p];
      if (g < 0 || g >= naggr) {
        free(cnt);
        c->bad_aggr = g;
        return cs_fail(PA_COARSE_AGGR, err, errlen, "part %d is in aggregate %d: expected 0 .. %d", p, g, naggr - 1);
      }
      cnt[g] += in->rowPos[p + 1] - in->rowPos[p];
    }
    for (int g = 0; g < naggr; ++g)
      if (cnt[g] <= 0) {
        free(cnt);
        c->bad_aggr = g;
        return cs_fail(PA_COARSE_AGGR, err, errlen, "aggregate %d is empty (no part with rows belongs to it)", g);
      }
    free(cnt);
  }
  c->m = m; c->k = k; c->naggr = naggr; c->nc = naggr * k; c->row_off = in->row_off;
  const size_t nn = (size_t)c->nc * c->nc;
  int rc = cs_chunks(in, c);
  if (!rc) {
    c->zv = (double*)malloc(((size_t)m * k + 1) * sizeof(double));
    c->E = (double*)calloc(nn, sizeof(double));
    c->Einv = (double*)malloc(nn * sizeof(double));
    if (!c->zv || !c->E || !c->Einv) rc = PA_COARSE_NOMEM;
  }
  if (rc) { pa_coarse_free(c); return cs_fail(rc, err, errlen, "out of host memory for the coarse space (%d unknowns)", naggr * k); }
  memcpy(c->zv, in->Vp + (size_t)in->row_off * k, (size_t)m * k * sizeof(double));
  rc = cs_assemble(in, c, threads);
  if (rc) { pa_coarse_free(c); return cs_fail(rc, err, errlen, "out of host memory"); }
  return PA_COARSE_OK;
}

/* ---- stage (b): E -> Einv ------------------------------------------------------------------------- */
int pa_coarse_invert(pa_coarse_t* c, int threads, char* err, size_t errlen) {
  if (!c || !c->E || !c->Einv || c->nc < 1 || c->k < 1) return cs_fail(PA_COARSE_ARG, err, errlen, "invalid arguments");
  const int rc = cs_invert(c, cs_threads(threads), err, errlen);
  if (rc) {
    const int ba = c->bad_aggr, bv = c->bad_vec;
    pa_coarse_free(c);
    c->bad_aggr = ba; c->bad_vec = bv;
  }
  return rc;
}

int pa_coarse_build(const pa_coarse_in_t* in, pa_coarse_t* c, char* err, size_t errlen) {
  if (!c) return PA_COARSE_ARG;
  memset(c, 0, sizeof(*c));
  c->bad_aggr = c->bad_vec = -1;
  if (!in || in->m < 0 || in->nparts < 1 || !in->rowPtr || !in->lcol || !in->val || !in->rowPos || !in->part_aggregate || !in->Vp)
    return cs_fail(PA_COARSE_ARG, err, errlen, "invalid arguments");
  const pa_coarse_share_in_t sh = {.m = in->m, .row_off = 0, .nparts = in->nparts, .part0 = 0, .np_loc = in->nparts,
                                   .rowPtr = in->rowPtr, .gcol = in->lcol, .val = in->val, .rowPos = in->rowPos,
                                   .part_aggregate = in->part_aggregate, .naggr = in->naggr, .k = in->k, .Vp = in->Vp,
                                   .max_dofs = in->max_dofs, .threads = in->threads};
  const int rc = pa_coarse_share(&sh, c, err, errlen);
  return rc ? rc : pa_coarse_invert(c, in->threads, err, errlen);
}

/* ---- default aggregates --------------------------------------------------------------------------- */
/* the np parts of the m rows whose first has the column id col_off; rowPos[p] - rowPos[0] is the first of those rows of
 * part p; an entry whose column is none of the m rows joins no two parts */
static int cs_default(int m, int np, const int* rowPtr, const int* col, int col_off, const int* rowPos, int k, int cap,
                      pa_coarse_kway_fn kway, int* part_aggregate, int* naggr, char* err, size_t errlen) {
  const int r0 = rowPos[0];
  if ((long long)np * k <= cap) {
    for (int p = 0; p < np; ++p) part_aggregate[p] = p;
    *naggr = np;
    return PA_COARSE_OK;
  }
  const int want = cap / k;
  if (want < 1) return cs_fail(PA_COARSE_CAP, err, errlen, "%d vectors do not fit the cap of %d coarse unknowns", k, cap);
  if (!kway) return cs_fail(PA_COARSE_ARG, err, errlen, "no partitioner for the quotient graph");
  /* quotient graph: parts p and q are neighbours when some a_ij joins them; the diagonal is stored */
  int* row_part = (int*)malloc((size_t)(m ? m : 1) * sizeof(int));
  int* qptr = (int*)calloc((size_t)np + 1, sizeof(int));
  int* mark = (int*)malloc((size_t)np * sizeof(int));
  int* qcol = NULL;
  int* map = NULL;
  int rc = PA_COARSE_OK;
  if (!row_part || !qptr || !mark) rc = PA_COARSE_NOMEM;
  if (!rc) {
    for (int p = 0; p < np; ++p) for (int i = rowPos[p] - r0; i < rowPos[p + 1] - r0; ++i) row_part[i] = p;
    for (int pass = 0; pass < 2 && !rc; ++pass) {
      for (int p = 0; p < np; ++p) mark[p] = -1;
      int n = 0;
      for (int p = 0; p < np; ++p) {
        const int first = n;
        mark[p] = p; if (pass) qcol[n] = p; ++n;
        for (int i = rowPos[p] - r0; i < rowPos[p + 1] - r0; ++i)
          for (int e = rowPtr[i]; e < rowPtr[i + 1]; ++e) {
            const int j = col[e] - col_off;
            if (j < 0 || j >= m) continue;
            const int q = row_part[j];
            if (mark[q] != p) { mark[q] = p; if (pass) qcol[n] = q; ++n; }
          }
        if (pass) {                                         /* ascending columns inside the row */
          for (int a = first + 1; a < n; ++a) {
            const int v = qcol[a]; int b = a;
            while (b > first && qcol[b - 1] > v) { qcol[b] = qcol[b - 1]; --b; }
            qcol[b] = v;
          }
        }
        qptr[p + 1] = n;
      }
      if (!pass) { qcol = (int*)malloc((size_t)(n ? n : 1) * sizeof(int)); if (!qcol) rc = PA_COARSE_NOMEM; }
    }
  }
  if (!rc && kway(np, qptr, qcol, want, part_aggregate))
    rc = cs_fail(PA_COARSE_ARG, err, errlen, "partitioning the quotient graph of %d parts into %d aggregates failed", np, want);
  else if (rc) cs_fail(rc, err, errlen, "out of host memory for the quotient graph of %d parts", np);
  if (!rc) {        /* number the aggregates that hold rows without gaps */
    map = (int*)malloc((size_t)want * sizeof(int));
    if (!map) rc = cs_fail(PA_COARSE_NOMEM, err, errlen, "out of host memory");
  }
  if (!rc) {
    for (int g = 0; g < want; ++g) map[g] = -1;
    for (int p = 0; p < np && !rc; ++p) {
      if (part_aggregate[p] < 0 || part_aggregate[p] >= want)
        rc = cs_fail(PA_COARSE_AGGR, err, errlen, "the partitioner put part %d into aggregate %d of %d", p, part_aggregate[p], want);
      else if (rowPos[p + 1] > rowPos[p]) map[part_aggregate[p]] = 0;
    }
  }
  if (!rc) {
    int n = 0;
    for (int g = 0; g < want; ++g) if (map[g] == 0) map[g] = n++;
    if (n == 0) { map[0] = 0; n = 1; }
    for (int p = 0; p < np; ++p) part_aggregate[p] = map[part_aggregate[p]] >= 0 ? map[part_aggregate[p]] : 0;
    *naggr = n;
  }
  free(row_part); free(qptr); free(mark); free(qcol); free(map);
  return rc;
}

int pa_coarse_default_aggregates(const pa_coarse_in_t* in, pa_coarse_kway_fn kway, int* part_aggregate, int* naggr,
                                 char* err, size_t errlen) {
  if (!in || !part_aggregate || !naggr || in->nparts < 1 || in->k < 1 || !in->rowPtr || !in->lcol || !in->rowPos)
    return cs_fail(PA_COARSE_ARG, err, errlen, "invalid arguments");
  return cs_default(in->m, in->nparts, in->rowPtr, in->lcol, 0, in->rowPos, in->k,
                    in->max_dofs > 0 ? in->max_dofs : PA_COARSE_MAX_DOFS, kway, part_aggregate, naggr, err, errlen);
}

int pa_coarse_default_aggregates_share(const pa_coarse_share_in_t* in, pa_coarse_kway_fn kway, int* local_aggregate,
                                       int* naggr_loc, char* err, size_t errlen) {
  if (!in || !local_aggregate || !naggr_loc || in->nparts < 1 || in->k < 1 || in->m < 0 || !in->rowPtr || !in->gcol || !in->rowPos ||
      in->part0 < 0 || in->np_loc < 0 || in->part0 + in->np_loc > in->nparts || in->rowPos[in->part0] != in->row_off ||
      in->rowPos[in->part0 + in->np_loc] != in->row_off + in->m)
    return cs_fail(PA_COARSE_ARG, err, errlen, "invalid arguments");
  const int np = in->nparts, npl = in->np_loc, k = in->k;
  const int cap = in->max_dofs > 0 ? in->max_dofs : PA_COARSE_MAX_DOFS;
  *naggr_loc = 0;
  if (npl == 0) return PA_COARSE_OK;
  if ((long long)np * k <= cap) {
    for (int p = 0; p < npl; ++p) local_aggregate[p] = p;
    *naggr_loc = npl;
    return PA_COARSE_OK;
  }
  if (cap / k < 1) return cs_fail(PA_COARSE_CAP, err, errlen, "%d vectors do not fit the cap of %d coarse unknowns", k, cap);
  long long share = (long long)(cap / k) * npl / np;
  if (share < 1) share = 1;
  /* (share <= npl: with share = npl the parts stay apart, otherwise the partitioner cuts the share's own quotient graph) */
  return cs_default(in->m, npl, in->rowPtr, in->gcol, in->row_off, in->rowPos + in->part0, k, (int)share * k, kway,
                    local_aggregate, naggr_loc, err, errlen);
}
