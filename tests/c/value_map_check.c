/*
 * value_map_check.c -- the value map of an SpMM plan (prealps_amd/csrc/spmm_plan.c: pa_spmm_plan_value_map), which
 * preAlps_OperatorUpdateValues uses to rewrite the values of the plan on the device, checked on the host against
 * the plan builders themselves.  On the panels of spmm_plan_dump.c (that file is included, its main renamed, so the
 * generators cannot drift apart), for the switch pairs that reach the window, the staged and the run plan at
 * strides 4, 8 and 16:
 *   - the plan cut from values v and the plan cut from other values v2 agree bytewise in every array but `val`
 *     and in every scalar: no decision of a builder reads a value;
 *   - val2[s] == (map[s] ? v2[map[s] - 1] : 0.0) for every slot s the upload copies, and the same for v;
 *   - every panel entry occurs in the map, exactly once in the window and the staged plan.
 * One line per case with the kind of plan reached; a non-zero exit and a line on stderr for every violation.
 * tests/test_value_map_cpu.py builds it with the host sanitizers.
 */
#define main spmm_plan_dump_main
#include "spmm_plan_dump.c"
#undef main

static int g_bad = 0;
#define BAD(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); g_bad = 1; } while (0)

static void check(const char* name, const panel_t* P, int part0, int part1, int ts, int cus, int staged, int runs) {
  const int nnz = P->rp[P->m];
  double* v2 = must(malloc(((size_t)nnz + 1) * sizeof(double)));
  for (int k = 0; k < nnz; ++k)      /* every value changes, none becomes zero */
    v2[k] = P->v[k] * (0.5 + (double)(((unsigned)k * 2654435761u) >> 20) / 4096.0) + 0.25;
  pa_spmm_plan_in_t in = {.m = P->m, .halo = P->halo, .part0 = part0, .part1 = part1, .row_off = P->row_off,
                          .rowPos = P->rowPos, .rowPtr = P->rp, .lcol = P->lcol, .val = P->v,
                          .ts = ts, .cus = cus, .want_staged = staged, .want_runs = runs};
  pa_spmm_plan_in_t in2 = in;
  in2.val = v2;
  pa_spmm_host_plan_t p1, p2;
  pa_spmm_value_map_t vm;
  char head[160];
  snprintf(head, sizeof(head), "%s ts=%d cus=%d staged_switch=%d runs_switch=%d", name, ts, cus, staged, runs);
  if (pa_spmm_plan_build(&in, &p1) || pa_spmm_plan_build(&in2, &p2) || pa_spmm_plan_value_map(&in, &vm)) {
    BAD("%s: a build failed", head);
    free(v2);
    return;
  }
  if (p1.m != p2.m || p1.nslices != p2.nslices || p1.nblk != p2.nblk || p1.n_interior != p2.n_interior ||
      p1.win_cap != p2.win_cap || p1.staged != p2.staged || p1.runs != p2.runs || p1.runs_cols != p2.runs_cols ||
      p1.stage_cap != p2.stage_cap || p1.sell_entries != p2.sell_entries || p1.stream_bytes != p2.stream_bytes)
    BAD("%s: the scalars of the plan depend on the values", head);
  for (int i = 0; i < PA_PL_COUNT; ++i) {
    const pa_plan_array_t* a = &p1.a[i];
    const pa_plan_array_t* b = &p2.a[i];
    if (!a->p != !b->p || a->n != b->n || a->n_alloc != b->n_alloc || a->elem != b->elem)
      BAD("%s: the shape of %s depends on the values", head, k_names[i]);
    else if (i != PA_PL_VAL && a->p && memcmp(a->p, b->p, a->n * a->elem))
      BAD("%s: %s depends on the values", head, k_names[i]);
  }
  const size_t n = p2.a[PA_PL_VAL].n;
  if (vm.n != n || vm.nslices != p2.nslices || vm.nblk != p2.nblk || vm.staged != p2.staged || vm.runs != p2.runs ||
      vm.runs_cols != p2.runs_cols)
    BAD("%s: the map describes another plan (%zu values, the plan has %zu)", head, vm.n, n);
  else {
    if (n % 64) BAD("%s: %zu stored values, not a multiple of 64", head, n);
    const double* val1 = (const double*)p1.a[PA_PL_VAL].p;
    const double* val2 = (const double*)p2.a[PA_PL_VAL].p;
    int* seen = must(calloc((size_t)nnz + 1, sizeof(int)));
    size_t wrong = 0, range = 0;
    for (size_t s = 0; s < n; ++s) {
      const uint32_t e = vm.map[s];
      if (e > (uint32_t)nnz) { ++range; continue; }
      if (e) ++seen[e - 1];
      const double w1 = e ? P->v[e - 1] : 0.0, w2 = e ? v2[e - 1] : 0.0;
      if (memcmp(&val1[s], &w1, sizeof(double)) || memcmp(&val2[s], &w2, sizeof(double))) ++wrong;
    }
    if (range) BAD("%s: %zu map entries point past the panel", head, range);
    if (wrong) BAD("%s: %zu stored values are not the gather of the map", head, wrong);
    size_t missing = 0, repeated = 0;
    for (int k = 0; k < nnz; ++k) { missing += seen[k] == 0; repeated += seen[k] > 1; }
    if (missing) BAD("%s: %zu panel entries are in no slot", head, missing);
    if (repeated && !p2.runs) BAD("%s: %zu panel entries are in more than one slot", head, repeated);
    free(seen);
    printf("%s: kind=%s slots=%zu entries=%d repeated=%zu\n", head, p2.runs ? "runs" : p2.staged ? "staged" : "window",
           n, nnz, repeated);
  }
  free(vm.map);
  pa_spmm_plan_free(&p1); pa_spmm_plan_free(&p2);
  free(v2);
}

static void check_panel(const char* name, const panel_t* P, int part0, int part1) {
  static const int strides[3] = {4, 8, 16}, cu_counts[2] = {1, 256};
  static const int switches[5][2] = {{-1, 1}, {1, 0}, {0, 1}, {-1, 0}, {-1, 2}};   /* (staged, runs) */
  for (int c = 0; c < 2; ++c) for (int t = 0; t < 3; ++t) for (int s = 0; s < 5; ++s)
    check(name, P, part0, part1, strides[t], cu_counts[c], switches[s][0], switches[s][1]);
}

int main(void) {
  (void)spmm_plan_dump_main;
  csr_t poisson = grid_matrix(12, 0, 1), nodes = grid_matrix(8, 1, 3), rnd = random_matrix(2048, 3, 5u);
  panel_t P = make_panel(&poisson, 5, 0, 5);
  check_panel("poisson12", &P, 0, 5);
  panel_free(&P);
  P = make_panel(&nodes, 7, 0, 7);
  check_panel("nodes8", &P, 0, 7);
  panel_free(&P);
  P = make_panel(&rnd, 3, 0, 3);
  check_panel("random2048", &P, 0, 3);
  panel_free(&P);
  P = make_panel(&poisson, 5, 1, 4);
  check_panel("poisson12_shard", &P, 1, 4);
  panel_free(&P);
  P = make_panel(&nodes, 7, 2, 5);
  check_panel("nodes8_shard", &P, 2, 5);
  panel_free(&P);
  csr_free(&poisson); csr_free(&nodes); csr_free(&rnd);
  return g_bad;
}
