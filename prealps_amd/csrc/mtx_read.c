/*
 * mtx_read.c -- MatrixMarket reader (utils/cplm_light/cplm_matcsr.c:96-243 of the reference).
 * coordinate real general|symmetric; 0-based files are detected from the first entry like the reference
 * does; symmetric files are expanded; repeated (i, j) entries are summed (in file order).  The file is
 * mapped and the host threads parse it in line-aligned pieces (an 81 M-nonzero matrix is 1.3 GB of text:
 * minutes through fscanf, seconds this way); values go through strtod, so they are the doubles
 * fscanf("%lf") would have produced.
 */
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/mman.h>

#include "mtx_read.h"
#include "pa_alloc.h"

typedef struct { int c; double v; } mm_ent_t;

static void mm_sort_row(mm_ent_t* e, int n, mm_ent_t* tmp) {   /* stable, by column */
  if (n <= 96) {
    for (int a = 1; a < n; ++a) { mm_ent_t x = e[a]; int q = a; while (q > 0 && e[q - 1].c > x.c) { e[q] = e[q - 1]; --q; } e[q] = x; }
    return;
  }
  int h = n / 2;
  mm_sort_row(e, h, tmp); mm_sort_row(e + h, n - h, tmp);
  memcpy(tmp, e, (size_t)h * sizeof(mm_ent_t));
  int i = 0, j = h, k = 0;
  while (i < h && j < n) e[k++] = (e[j].c < tmp[i].c) ? e[j++] : tmp[i++];
  while (i < h) e[k++] = tmp[i++];
}

/* one "i j v" line starting at p (p < end); returns the position behind the line, NULL on a bad line */
static const char* mm_parse_line(const char* p, const char* end, int* I, int* J, double* V) {
  long val[2];
  for (int f = 0; f < 2; ++f) {
    while (p < end && (*p == ' ' || *p == '\t')) ++p;
    int neg = 0;
    if (p < end && (*p == '-' || *p == '+')) { neg = *p == '-'; ++p; }
    if (p >= end || *p < '0' || *p > '9') return NULL;
    long x = 0;
    while (p < end && *p >= '0' && *p <= '9') { x = 10 * x + (*p - '0'); ++p; }
    val[f] = neg ? -x : x;
  }
  while (p < end && (*p == ' ' || *p == '\t')) ++p;
  /* the number's characters, NUL terminated for strtod (never reads past the mapping) */
  char buf[64];
  int l = 0;
  while (p + l < end && l < 63 && p[l] != '\n' && p[l] != '\r' && p[l] != ' ' && p[l] != '\t') { buf[l] = p[l]; ++l; }
  buf[l] = 0;
  if (l == 0) return NULL;
  char* stop = NULL;
  *V = strtod(buf, &stop);
  if (stop == buf) return NULL;
  p += l;
  while (p < end && *p != '\n') ++p;
  *I = (int)val[0]; *J = (int)val[1];
  return p < end ? p + 1 : end;
}

void pa_mtx_free(pa_mtx_t* m) {
  free(m->rowPtr); free(m->colInd); free(m->val);
  memset(m, 0, sizeof(*m));
}

/* every failure leaves through `done`, which releases whatever is set */
#define MM_FAIL(code, ...) do { rc = (code); if (err && errlen) snprintf(err, errlen, __VA_ARGS__); goto done; } while (0)
#define MM_TRACE(what) do { if (trace) { double n_ = omp_get_wtime(); fprintf(stderr, "[setup] %-28s %.3f s\n", what, n_ - t_tr); t_tr = n_; } } while (0)

int pa_mtx_read(const char* file, int threads, int trace, pa_mtx_t* out, char* err, size_t errlen) {
  int rc = PA_MTX_OK;
  FILE* fd = NULL;
  const char* map = NULL; long fsize = 0;
  const char** cut = NULL; long long* first = NULL;
  int* I = NULL; int* J = NULL; double* V = NULL;
  int* hist = NULL; int* rp = NULL; mm_ent_t* ent = NULL; int* len = NULL;
  int* rp2 = NULL; int* ci = NULL; double* vv = NULL;
  memset(out, 0, sizeof(*out));
  if (threads < 1) threads = 1;
  fd = fopen(file, "r");
  if (!fd) MM_FAIL(PA_MTX_OPEN, "Impossible to open the file %s", file);
  char line[1025], banner[64], mtx[64], crd[64], dt[64], sym[64];
  if (!fgets(line, sizeof(line), fd) ||
      sscanf(line, "%63s %63s %63s %63s %63s", banner, mtx, crd, dt, sym) != 5 ||
      strcasecmp(banner, "%%MatrixMarket") || strcasecmp(mtx, "matrix") ||
      strcasecmp(crd, "coordinate") || strcasecmp(dt, "real") ||
      (strcasecmp(sym, "general") && strcasecmp(sym, "symmetric")))
    MM_FAIL(PA_MTX_FORMAT, "Only sparse real < symmetric | general > matrix are currently supported (%s)", file);
  const int is_sym = !strcasecmp(sym, "symmetric");
  do { if (!fgets(line, sizeof(line), fd)) MM_FAIL(PA_MTX_FORMAT, "truncated file %s", file); } while (line[0] == '%');
  int M = 0, Nc = 0; long long nz = 0;
  if (sscanf(line, "%d %d %lld", &M, &Nc, &nz) != 3 || M < 1 || Nc != M || nz < 1)
    MM_FAIL(PA_MTX_FORMAT, "[LoadMatrixMarket] Error: Invalid matrix dimensions in %s", file);
  long body = ftell(fd);
  fseek(fd, 0, SEEK_END);
  fsize = ftell(fd);
  if (body < 0 || fsize <= body) MM_FAIL(PA_MTX_FORMAT, "truncated file %s", file);
  map = (const char*)mmap(NULL, (size_t)fsize, PROT_READ, MAP_PRIVATE, fileno(fd), 0);
  fclose(fd); fd = NULL;
  if (map == MAP_FAILED) { map = NULL; MM_FAIL(PA_MTX_OPEN, "cannot map %s", file); }
  (void)madvise((void*)map, (size_t)fsize, MADV_SEQUENTIAL);
  const char* beg = map + body;
  const char* end = map + fsize;
  double t_tr = omp_get_wtime();
  int T = threads;
  if ((long long)T > nz / 4096 + 1) T = (int)(nz / 4096 + 1);
  if (T < 1) T = 1;
  /* pieces that start behind a newline */
  cut = (const char**)malloc(((size_t)T + 1) * sizeof(char*));
  first = (long long*)calloc((size_t)T + 1, sizeof(long long));
  I = (int*)malloc((size_t)nz * sizeof(int));
  J = (int*)malloc((size_t)nz * sizeof(int));
  V = (double*)malloc((size_t)nz * sizeof(double));
  if (!cut || !first || !I || !J || !V) MM_FAIL(PA_MTX_NOMEM, "out of host memory for %lld entries", nz);
  cut[0] = beg; cut[T] = end;
  for (int t = 1; t < T; ++t) {
    const char* p = beg + (size_t)((double)(end - beg) * t / T);
    if (p < cut[t - 1]) p = cut[t - 1];
    const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
    cut[t] = nl ? nl + 1 : end;
  }
  /* lines per piece (blank lines do not count) */
#pragma omp parallel for num_threads(T) schedule(static, 1)
  for (int t = 0; t < T; ++t) {
    long long n = 0;
    const char* p = cut[t];
    while (p < cut[t + 1]) {
      const char* nl = (const char*)memchr(p, '\n', (size_t)(cut[t + 1] - p));
      const char* le = nl ? nl : cut[t + 1];
      const char* q = p;
      while (q < le && (*q == ' ' || *q == '\t' || *q == '\r')) ++q;
      if (q < le && *q != '%') ++n;           /* (blank lines and comment lines inside the body do not count) */
      p = nl ? nl + 1 : cut[t + 1];
    }
    first[t + 1] = n;
  }
  for (int t = 0; t < T; ++t) first[t + 1] += first[t];
  MM_TRACE("  mtx: count lines");
  const int bad = first[T] < nz;     /* (extra lines behind the nz announced are ignored, like fscanf would) */
  long long bad_line = -1;
  if (!bad) {
#pragma omp parallel for num_threads(T) schedule(static, 1)
    for (int t = 0; t < T; ++t) {
      long long k = first[t];
      const char* p = cut[t];
      while (p && p < cut[t + 1] && k < nz) {
        const char* q = p;
        while (q < cut[t + 1] && (*q == ' ' || *q == '\t' || *q == '\r')) ++q;
        if (q < cut[t + 1] && *q == '\n') { p = q + 1; continue; }
        if (q >= cut[t + 1]) break;
        if (*q == '%') {                         /* a comment line in the body: skipped */
          const char* nl = (const char*)memchr(q, '\n', (size_t)(cut[t + 1] - q));
          p = nl ? nl + 1 : cut[t + 1];
          continue;
        }
        p = mm_parse_line(q, cut[t + 1], &I[k], &J[k], &V[k]);
        if (!p) {
#pragma omp critical
          { if (bad_line < 0 || k < bad_line) bad_line = k; }
          break;
        }
        ++k;
      }
    }
  }
  munmap((void*)map, (size_t)fsize); map = NULL;
  MM_TRACE("  mtx: parse");
  if (bad || bad_line >= 0) MM_FAIL(PA_MTX_ENTRY, "bad entry %lld in %s", bad ? first[T] : bad_line, file);
  const int base = (I[0] == 0 || J[0] == 0) ? 0 : 1;
  int oob = 0;
#pragma omp parallel for num_threads(threads) schedule(static) reduction(|| : oob)
  for (long long k = 0; k < nz; ++k) {
    I[k] -= base; J[k] -= base;
    if (I[k] < 0 || I[k] >= M || J[k] < 0 || J[k] >= M) oob = 1;
  }
  if (oob) MM_FAIL(PA_MTX_ENTRY, "index out of range in %s", file);
  /* row histograms per thread (thread t owns entries [t nz / T, (t+1) nz / T)): positions that keep
   * the file order inside every row, without atomics */
  int TH = threads;
  while (TH > 1 && (size_t)TH * (size_t)M * sizeof(int) > ((size_t)1 << 30)) TH /= 2;
  hist = (int*)calloc((size_t)TH * (size_t)M, sizeof(int));
  rp = (int*)malloc(((size_t)M + 1) * sizeof(int));
  if (!hist || !rp) MM_FAIL(PA_MTX_NOMEM, "out of host memory");
#pragma omp parallel for num_threads(TH) schedule(static, 1)
  for (int t = 0; t < TH; ++t) {
    int* h = hist + (size_t)t * M;
    long long k0 = nz * t / TH, k1 = nz * (t + 1) / TH;
    for (long long k = k0; k < k1; ++k) { h[I[k]]++; if (is_sym && I[k] != J[k]) h[J[k]]++; }
  }
  long long tot = 0;
  for (int i = 0; i < M; ++i) {
    rp[i] = (int)tot;
    for (int t = 0; t < TH; ++t) { int c = hist[(size_t)t * M + i]; hist[(size_t)t * M + i] = (int)tot; tot += c; }
    if (tot > 2147483000LL) MM_FAIL(PA_MTX_FORMAT, "%s has too many nonzeros for int32 indices", file);
  }
  rp[M] = (int)tot;
  ent = (mm_ent_t*)pa_big_alloc((size_t)(tot ? tot : 1) * sizeof(mm_ent_t));
  if (!ent) MM_FAIL(PA_MTX_NOMEM, "out of host memory for %lld entries", tot);
#pragma omp parallel for num_threads(TH) schedule(static, 1)
  for (int t = 0; t < TH; ++t) {
    int* h = hist + (size_t)t * M;
    long long k0 = nz * t / TH, k1 = nz * (t + 1) / TH;
    for (long long k = k0; k < k1; ++k) {
      ent[h[I[k]]].c = J[k]; ent[h[I[k]]++].v = V[k];
      if (is_sym && I[k] != J[k]) { ent[h[J[k]]].c = I[k]; ent[h[J[k]]++].v = V[k]; }
    }
  }
  free(hist); free(I); free(J); free(V);   /* (the largest arrays go before the next ones come) */
  hist = NULL; I = NULL; J = NULL; V = NULL;
  MM_TRACE("  mtx: rows (histograms, scatter)");
  /* sort every row by column (stable), sum repeated entries, compact */
  len = (int*)malloc((size_t)M * sizeof(int));
  if (!len) MM_FAIL(PA_MTX_NOMEM, "out of host memory");
  int no_mem = 0;        /* a thread could not get its sort buffer: the rows it met stay unsorted, the build fails */
#pragma omp parallel num_threads(threads)
  {
    int cap = 256;
    mm_ent_t* tmp = (mm_ent_t*)malloc((size_t)cap * sizeof(mm_ent_t));
#pragma omp for schedule(dynamic, 1024)
    for (int i = 0; i < M; ++i) {
      int k0 = rp[i], n = rp[i + 1] - k0;
      if (n / 2 + 1 > cap || !tmp) { cap = n > cap ? n : cap; free(tmp); tmp = (mm_ent_t*)malloc((size_t)cap * sizeof(mm_ent_t)); }
      int sorted = 1;
      for (int k = 1; k < n && sorted; ++k) sorted = ent[k0 + k - 1].c <= ent[k0 + k].c;
      if (!sorted && !tmp) {
#pragma omp atomic write
        no_mem = 1;
      }
      if (!sorted && tmp) mm_sort_row(ent + k0, n, tmp);
      int o = 0;
      for (int k = 0; k < n; ++k) {
        if (o > 0 && ent[k0 + k].c == ent[k0 + o - 1].c) ent[k0 + o - 1].v += ent[k0 + k].v;
        else ent[k0 + o++] = ent[k0 + k];
      }
      len[i] = o;
    }
    free(tmp);
  }
  if (no_mem) MM_FAIL(PA_MTX_NOMEM, "out of host memory while sorting the rows of %s", file);
  rp2 = (int*)malloc(((size_t)M + 1) * sizeof(int));
  long long nnz = 0;
  for (int i = 0; rp2 && i < M; ++i) { rp2[i] = (int)nnz; nnz += len[i]; }
  ci = (int*)pa_big_alloc((size_t)(nnz ? nnz : 1) * sizeof(int));
  vv = (double*)pa_big_alloc((size_t)(nnz ? nnz : 1) * sizeof(double));
  if (!rp2 || !ci || !vv) MM_FAIL(PA_MTX_NOMEM, "out of host memory");
  rp2[M] = (int)nnz;
#pragma omp parallel for num_threads(threads) schedule(static)
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < len[i]; ++k) { ci[rp2[i] + k] = ent[rp[i] + k].c; vv[rp2[i] + k] = ent[rp[i] + k].v; }
  MM_TRACE("  mtx: sort + compact");
  out->N = M; out->rowPtr = rp2; out->colInd = ci; out->val = vv;
  rp2 = NULL; ci = NULL; vv = NULL;
done:
  if (fd) fclose(fd);
  if (map) munmap((void*)map, (size_t)fsize);
  free(cut); free(first); free(I); free(J); free(V); free(hist); free(rp); free(ent); free(len);
  free(rp2); free(ci); free(vv);
  return rc;
}
