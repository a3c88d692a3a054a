/*
 * bj_share.c -- the classes of identical diagonal blocks (bj_share.h): one hash per band (parallel over the
 * blocks), the eligible blocks sorted by (hash, rows, bandwidth, number), every block of a run compared with the
 * run's first (parallel), and the few that differ from it -- blocks that only collide -- sorted out one after the
 * other against the representatives their run has so far.  And the pair tasks of a launch list, from the classes.
 */
#include <assert.h>
#include <stdlib.h>
#include <string.h>

#include "bj_share.h"

typedef struct { unsigned long long h; int nrows, bw, p; } share_key_t;

/* the 64-bit words of a band, mixed one after the other (the words are read through memcpy: no aliasing) */
static unsigned long long band_hash(const double* band, size_t n) {
  unsigned long long h = 0x9E3779B97F4A7C15ull ^ (unsigned long long)n;
  for (size_t i = 0; i < n; ++i) {
    unsigned long long x;
    memcpy(&x, band + i, sizeof(x));
    h = (h ^ x) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
  }
  return h;
}

static int key_cmp(const void* a, const void* b) {
  const share_key_t* x = (const share_key_t*)a;
  const share_key_t* y = (const share_key_t*)b;
  if (x->h != y->h) return x->h < y->h ? -1 : 1;
  if (x->nrows != y->nrows) return x->nrows < y->nrows ? -1 : 1;
  if (x->bw != y->bw) return x->bw < y->bw ? -1 : 1;
  return x->p < y->p ? -1 : (x->p > y->p ? 1 : 0);
}

static size_t band_bytes(const share_key_t* k) { return (size_t)k->nrows * ((size_t)k->bw + 1) * sizeof(double); }

int pa_bj_share_classes(const pa_bj_share_in_t* in, int* rep, int* nclass) {
  const int np = in->np, threads = in->threads > 0 ? in->threads : 1;
  int ne = 0;
  for (int p = 0; p < np; ++p) { rep[p] = p; ne += in->eligible[p] && in->bands[p]; }
  *nclass = np;
  if (ne < 2) return 0;
  share_key_t* key = (share_key_t*)malloc((size_t)ne * sizeof(share_key_t));
  int* first = (int*)malloc((size_t)ne * sizeof(int));      /* position of the first key of a key's run */
  int* reps = (int*)malloc((size_t)ne * sizeof(int));       /* the representatives of the run at hand, ascending */
  char* same = (char*)malloc((size_t)ne);                   /* 1: the same bytes as the run's first */
  if (!key || !first || !reps || !same) { free(key); free(first); free(reps); free(same); return -1; }
  ne = 0;
  for (int p = 0; p < np; ++p)
    if (in->eligible[p] && in->bands[p]) { key[ne].nrows = in->nrows[p]; key[ne].bw = in->bw[p]; key[ne].p = p; ++ne; }
#pragma omp parallel for num_threads(threads) schedule(dynamic, 16)
  for (int i = 0; i < ne; ++i)
    key[i].h = band_hash(in->bands[key[i].p], (size_t)key[i].nrows * ((size_t)key[i].bw + 1)) & in->hash_mask;
  qsort(key, (size_t)ne, sizeof(share_key_t), key_cmp);
  for (int i = 0; i < ne; ++i)
    first[i] = i > 0 && key[i].h == key[i - 1].h && key[i].nrows == key[i - 1].nrows && key[i].bw == key[i - 1].bw ? first[i - 1] : i;
#pragma omp parallel for num_threads(threads) schedule(dynamic, 16)
  for (int i = 0; i < ne; ++i)
    same[i] = first[i] != i && !memcmp(in->bands[key[i].p], in->bands[key[first[i]].p], band_bytes(&key[i]));
  /* a run in ascending block order: its first is a representative; a block with other bytes than the first is
   * compared with the later representatives, oldest first, and becomes one itself if it equals none */
  int nreps = 0, shared = 0;
  for (int i = 0; i < ne; ++i) {
    if (first[i] == i) { nreps = 0; reps[nreps++] = key[i].p; continue; }
    int r = same[i] ? reps[0] : -1;
    for (int k = 1; k < nreps && r < 0; ++k)
      if (!memcmp(in->bands[key[i].p], in->bands[reps[k]], band_bytes(&key[i]))) r = reps[k];
    if (r < 0) reps[nreps++] = key[i].p;
    else { rep[key[i].p] = r; ++shared; }
  }
  *nclass = np - shared;
  free(key); free(first); free(reps); free(same);
  return 0;
}

int pa_bj_pair_tasks(int np, const int* list, int count, const int* rep, const int* nrows, const int* bw, int* tasks,
                     int* ntasks, int* paired) {
  *ntasks = 0; *paired = 0;
  if (count <= 0) return 0;
  int* open = (int*)malloc((size_t)(np > 0 ? np : 1) * sizeof(int));      /* per class: its task that waits for a partner */
  if (!open) return -1;
  for (int p = 0; p < np; ++p) open[p] = -1;
  int nt = 0, np2 = 0;
  for (int i = 0; i < count; ++i) {
    const int p = list[i];
    assert(p >= 0 && p < np);
    const int r = rep[p];
    assert(r >= 0 && r < np && nrows[r] == nrows[p] && bw[r] == bw[p]);
    if (open[r] >= 0) { tasks[2 * open[r] + 1] = i; open[r] = -1; np2 += 2; }
    else { tasks[2 * nt] = i; tasks[2 * nt + 1] = -1; open[r] = nt++; }
  }
  free(open);
  *ntasks = nt; *paired = np2;
  return 0;
}
