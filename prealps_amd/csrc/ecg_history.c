/*
 * ecg_history.c -- ring bookkeeping, Gram update and the scaled pivoted Cholesky of the solution history
 * (ecg_history.h states the rule and its limits).  Pure host arithmetic: <math.h> and nothing else.
 */
#include <math.h>
#include "ecg_history.h"

#define LDG PA_HIST_MAX

int pa_hist_capacity_ok(int cap) { return cap >= 1 && cap <= PA_HIST_MAX; }

void pa_hist_clear(pa_hist_t* h) {
  h->count = 0; h->head = 0;
  for (int e = 0; e < LDG * LDG; ++e) h->G[e] = 0.0;
}

int pa_hist_init(pa_hist_t* h, int cap) {
  if (!h || !pa_hist_capacity_ok(cap)) return PA_HIST_BAD_ARGS;
  h->cap = cap;
  pa_hist_clear(h);
  return PA_HIST_OK;
}

int pa_hist_slot(const pa_hist_t* h, int i) {
  if (i < 0 || i >= h->count) return -1;
  return (h->head + i) % h->cap;
}

int pa_hist_append(pa_hist_t* h, int q, const double* DO, int ldo, const double* DN, int ldn, int* slots) {
  if (!h || q < 1 || q > PA_HIST_MAX || !DN || ldn < q || !slots || (h->count > 0 && (!DO || ldo < h->count)))
    return PA_HIST_BAD_ARGS;
  for (int j = 0; j < q; ++j) {
    const double d = DN[j + (long)j * ldn];
    if (!(d - d == 0.0)) return PA_HIST_BAD_GRAM;
  }
  /* owner[s]: the new column in slot s, -1: the column that was there before the call (or none) */
  int owner[PA_HIST_MAX];
  for (int s = 0; s < PA_HIST_MAX; ++s) owner[s] = -1;
  const int first = q > h->cap ? q - h->cap : 0;
  for (int j = 0; j < q; ++j) slots[j] = -1;
  for (int j = first; j < q; ++j) {
    int s;
    if (h->count < h->cap) s = h->count++;                        /* (head stays 0 until the ring is full) */
    else { s = h->head; h->head = (h->head + 1) % h->cap; }       /* the oldest column leaves */
    owner[s] = j; slots[j] = s;
  }
  /* the rows and columns of the slots taken: an evicted column's entries are all overwritten here */
  for (int j = first; j < q; ++j) {
    const int sj = slots[j];
    for (int s = 0; s < h->count; ++s) {
      const int a = owner[s];
      double v;
      if (a < 0) v = DO[s + (long)j * ldo];
      else v = a <= j ? DN[a + (long)j * ldn] : DN[j + (long)a * ldn];
      h->G[s + LDG * sj] = v;
      h->G[sj + LDG * s] = v;
    }
  }
  return PA_HIST_OK;
}

int pa_hist_set_gram(pa_hist_t* h, const double* D, int ldd) {
  if (!h || (h->count > 0 && (!D || ldd < h->count))) return PA_HIST_BAD_ARGS;
  for (int j = 0; j < h->count; ++j)
    for (int i = 0; i <= j; ++i) {
      const double v = D[i + (long)j * ldd];
      h->G[i + LDG * j] = v;
      h->G[j + LDG * i] = v;
    }
  return PA_HIST_OK;
}

int pa_hist_factor_solve(int K, const double* Gs, int q, const double* gs, double rtol, double* cs, int* piv) {
  /* R: the rows of the upper factor in the order the pivots were taken, R[r][j] for every column j (original index) */
  double R[PA_HIST_MAX][PA_HIST_MAX], dg[PA_HIST_MAX];
  int taken[PA_HIST_MAX];
  int rank = 0;
  for (int j = 0; j < K; ++j) { dg[j] = Gs[j + (long)j * K]; taken[j] = 0; }
  while (rank < K) {
    int p = -1;
    double best = rtol;
    for (int j = 0; j < K; ++j)
      if (!taken[j] && dg[j] > best) { best = dg[j]; p = j; }       /* (the first of equal pivots: ring order) */
    if (p < 0) break;
    const double rpp = sqrt(best);
    for (int j = 0; j < K; ++j) R[rank][j] = 0.0;
    R[rank][p] = rpp;
    taken[p] = 1; piv[rank] = p;
    for (int j = 0; j < K; ++j) {
      if (taken[j]) continue;
      double v = Gs[p + (long)j * K];
      for (int r = 0; r < rank; ++r) v -= R[r][p] * R[r][j];
      v /= rpp;
      R[rank][j] = v;
      dg[j] -= v * v;
    }
    ++rank;
  }
  /* R^T y = gs[piv], R cs[piv] = y on the leading rank x rank block, whose entry (r, i) is R[r][piv[i]], r <= i */
  for (int c = 0; c < q; ++c) {
    double y[PA_HIST_MAX];
    for (int i = 0; i < rank; ++i) {
      double v = gs[piv[i] + (long)c * K];
      for (int r = 0; r < i; ++r) v -= R[r][piv[i]] * y[r];
      y[i] = v / R[i][piv[i]];
    }
    for (int j = 0; j < K; ++j) cs[j + (long)c * K] = 0.0;
    for (int i = rank - 1; i >= 0; --i) {
      double v = y[i];
      for (int r = i + 1; r < rank; ++r) v -= R[i][piv[r]] * cs[piv[r] + (long)c * K];
      cs[piv[i] + (long)c * K] = v / R[i][piv[i]];
    }
  }
  return rank;
}

int pa_hist_project(const pa_hist_t* h, int q, const double* g, double rtol, double* c, int* rank, double* captured) {
  if (!h || q < 1 || q > PA_HIST_MAX || !c || !rank || (h->count > 0 && !g)) return PA_HIST_BAD_ARGS;
  const int K = h->count;
  *rank = 0;
  for (int j = 0; captured && j < q; ++j) captured[j] = 0.0;
  if (K == 0) return PA_HIST_OK;
  if (!(rtol > 0.0)) rtol = PA_HIST_RTOL_DEFAULT;
  double s[PA_HIST_MAX], Gs[PA_HIST_MAX * PA_HIST_MAX], gs[PA_HIST_MAX * PA_HIST_MAX], cs[PA_HIST_MAX * PA_HIST_MAX];
  int slot[PA_HIST_MAX], piv[PA_HIST_MAX];
  double dmax = 0.0;
  for (int i = 0; i < K; ++i) {
    slot[i] = pa_hist_slot(h, i);
    for (int j = 0; j < K; ++j) {
      const double v = h->G[slot[i] + LDG * ((h->head + j) % h->cap)];
      if (!(v - v == 0.0)) return PA_HIST_BAD_GRAM;
    }
    const double d = h->G[slot[i] + LDG * slot[i]];
    if (d > dmax) dmax = d;
    s[i] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
  }
  if (!(dmax > 0.0)) return PA_HIST_BAD_GRAM;
  for (int j = 0; j < K; ++j)
    for (int i = 0; i < K; ++i) {
      const double v = i == j ? (s[i] > 0.0 ? 1.0 : 0.0) : (h->G[slot[i] + LDG * slot[j]] * s[i]) * s[j];
      Gs[i + K * j] = v;
    }
  /* (symmetric in bits: G is, and (G_ij s_i) s_j against (G_ji s_j) s_i differ, so the upper triangle is mirrored) */
  for (int j = 0; j < K; ++j) for (int i = j + 1; i < K; ++i) Gs[i + K * j] = Gs[j + K * i];
  for (int cc = 0; cc < q; ++cc) for (int i = 0; i < K; ++i) gs[i + K * cc] = g[i + (long)K * cc] * s[i];
  *rank = pa_hist_factor_solve(K, Gs, q, gs, rtol, cs, piv);
  for (int cc = 0; cc < q; ++cc) {
    double cap = 0.0;
    for (int i = 0; i < K; ++i) {
      const double v = cs[i + K * cc] * s[i];
      c[i + (long)K * cc] = v;
      cap += v * g[i + (long)K * cc];
    }
    if (captured) captured[cc] = cap;
  }
  return PA_HIST_OK;
}

int pa_hist_red_layout(int entry, int K, int q, pa_hist_red_t* l) {
  if (!l || K < 0 || K > PA_HIST_MAX) return PA_HIST_BAD_ARGS;
  pa_hist_red_t n;
  const int sums = 1, first = sums + PA_HIST_MAX, second = first + PA_HIST_MAX * PA_HIST_MAX;
  if (entry == PA_HIST_RED_REFRESH) {
    if (K < 1) return PA_HIST_BAD_ARGS;
    n.off_a = first; n.rows_a = K; n.cols_a = K; n.off_b = second; n.rows_b = 0; n.cols_b = 0; n.words = second;
  } else {
    if (q < 1 || q > PA_HIST_MAX) return PA_HIST_BAD_ARGS;
    if (entry == PA_HIST_RED_PROJECT) {
      n.off_a = sums; n.rows_a = 1; n.cols_a = q; n.off_b = first; n.rows_b = K; n.cols_b = q; n.words = second;
    } else if (entry == PA_HIST_RED_APPEND) {
      n.off_a = first; n.rows_a = K; n.cols_a = q; n.off_b = second; n.rows_b = q; n.cols_b = q; n.words = PA_HIST_RED_WORDS;
    } else return PA_HIST_BAD_ARGS;
  }
  *l = n;
  return PA_HIST_OK;
}
