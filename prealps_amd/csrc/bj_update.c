/*
 * bj_update.c -- numeric refactorisation of the block-Jacobi preconditioner in place
 * (preAlps_BlockJacobiUpdateValues): new values on the create's pattern reach the bands through the band map
 * (bj_band_map.h), and the create's launches run again on the create's layout (bj_priv.h: pa_bj_t.lay).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bj_priv.h"

#define BJU_FAIL(...) pa_fail_at("preAlps_BlockJacobiUpdateValues", __VA_ARGS__)

static void bj_band_map_release(pa_bj_t* s) {
  pa_rt_free(s->d_bm_src); pa_rt_free(s->d_bm_dst); pa_rt_free(s->d_bm_chunk_blk); pa_rt_free(s->d_bm_chunk_first);
  pa_rt_free(s->d_boff); pa_rt_free(s->d_slist); pa_rt_free(s->d_blist); pa_rt_free(s->d_fail);
  s->d_bm_src = s->d_bm_dst = s->d_bm_chunk_first = NULL; s->d_bm_chunk_blk = s->d_slist = s->d_blist = s->d_fail = NULL;
  s->d_boff = NULL;
}

/* The band map of the current preconditioner on the device, with the layout's band offsets and the launch lists
 * of pa_k_bj_factor / pa_k_bj_factor_big: cut once per create. */
static int bj_ensure_band_map(pa_bj_t* s, const pa_operator_info_t* op) {
  if (s->d_bm_src) return 0;
  const int np = s->np;
  const pa_bj_layout_t* L = &s->lay;
  const double t0 = pa_wtime();
  pa_bj_band_map_in_t in = {.np = np, .rowPtr = op->A.rowPtr, .colInd = op->A.colInd, .row0 = s->h_row0, .nrows = s->h_nrows,
                            .grow0 = s->h_grow0, .bw = s->h_bw, .order = s->h_map_f, .is_nd = s->h_is_nd,
                            .wmax = s->dev_wmax, .chunk = 1024};
  pa_bj_band_map_t bm;
  const int brc = pa_bj_band_map_build(&in, &bm);
  if (brc == -2)
    return BJU_FAIL("the band of block %d (%d rows, bandwidth %d) has 2^32 entries or more: free and create instead",
                    bm.bad_block, s->h_nrows[bm.bad_block], s->h_bw[bm.bad_block]);
  if (brc == -3) return BJU_FAIL("block %d of the panel no longer has the pattern the preconditioner was created from", bm.bad_block);
  if (brc) return BJU_FAIL("out of host memory for the band map");
  ++s->bm_builds;
  int rc = 0;
  s->d_bm_src = (unsigned*)pa_rt_malloc((bm.n ? bm.n : 1) * sizeof(unsigned));
  s->d_bm_dst = (unsigned*)pa_rt_malloc((bm.n ? bm.n : 1) * sizeof(unsigned));
  s->d_bm_chunk_blk = (int*)pa_rt_malloc((bm.nchunks ? bm.nchunks : 1) * sizeof(int));
  s->d_bm_chunk_first = (unsigned*)pa_rt_malloc((bm.nchunks + 1) * sizeof(unsigned));
  s->d_boff = (long long*)pa_rt_malloc(((size_t)np + 1) * sizeof(long long));
  s->d_slist = (int*)pa_rt_malloc((L->ns ? L->ns : 1) * sizeof(int));
  s->d_blist = (int*)pa_rt_malloc((L->nbig ? L->nbig : 1) * sizeof(int));
  s->d_fail = (int*)pa_rt_malloc(sizeof(int));
  if (!s->d_bm_src || !s->d_bm_dst || !s->d_bm_chunk_blk || !s->d_bm_chunk_first || !s->d_boff || !s->d_slist ||
      !s->d_blist || !s->d_fail ||
      pa_rt_h2d(s->d_bm_src, bm.src, bm.n * sizeof(unsigned)) || pa_rt_h2d(s->d_bm_dst, bm.dst, bm.n * sizeof(unsigned)) ||
      pa_rt_h2d(s->d_bm_chunk_blk, bm.chunk_blk, bm.nchunks * sizeof(int)) ||
      pa_rt_h2d(s->d_bm_chunk_first, bm.chunk_first, (bm.nchunks + 1) * sizeof(unsigned)) ||
      pa_rt_h2d(s->d_boff, L->boff, ((size_t)np + 1) * sizeof(long long)) ||
      pa_rt_h2d(s->d_slist, L->slist, (size_t)L->ns * sizeof(int)) || pa_rt_h2d(s->d_blist, L->blist, (size_t)L->nbig * sizeof(int))) {
    rc = BJU_FAIL("uploading the band map (%zu entries) failed: %s", bm.n, pa_rt_error());
    bj_band_map_release(s);
  }
  if (!rc) {
    s->bm_n = bm.n; s->bm_nchunks = bm.nchunks; s->bm_bytes = pa_bj_band_map_bytes(&bm);
    s->upd_map_s = pa_wtime() - t0;
  }
  pa_bj_band_map_free(&bm);
  return rc;
}

/* The band blocks: panel values up in one copy, bands assembled on the device through the map, then the
 * factorisation and layout launches of the create on the create's lists, offsets and records.  Every kernel
 * writes, for the same (rows, bandwidth, wide), the positions it wrote at the create -- k_bj_factor and
 * k_bj_layout_big the in-band entries of the plain records, k_bj_g4_setup and k_bj_pairs every element of a
 * block's second record -- so the zero background of the create survives and nothing is cleared.
 * *spd_fail: 1 + local position of a non-positive pivot.  Returns non-zero with the error reported;
 * *wrote tells whether the factor may have been written to by then. */
static int bj_refactor_bands(pa_bj_t* s, const pa_operator_info_t* op, int* wrote, int* spd_fail) {
  const size_t lnnz = (size_t)op->A.rowPtr[s->m], btot = s->lay.btot;
  double* d_pv = (double*)pa_rt_malloc((lnnz ? lnnz : 1) * sizeof(double));
  double* d_band = (double*)pa_rt_malloc((btot ? btot : 1) * sizeof(double));
  void* e0 = pa_rt_event_create();
  void* e1 = pa_rt_event_create();
  int rc = 0, fail = 0;
  if (!d_pv || !d_band || !e0 || !e1)
    rc = BJU_FAIL("no device memory for the panel values (%zu) and the bands (%zu entries): %s", lnnz, btot, pa_rt_error());
  if (!rc) {
    /* behind the applies already queued on the library stream; the copy returns when it has read A->val */
    const double t0 = pa_wtime();
    if (pa_rt_h2d(d_pv, op->A.val, lnnz * sizeof(double))) rc = BJU_FAIL("uploading the panel values failed: %s", pa_rt_error());
    s->upd_copy_s = pa_wtime() - t0;
  }
  if (!rc) {
    *wrote = 1;
    if (pa_rt_event_record(e0) || pa_rt_memset(d_band, 0, btot * sizeof(double)) || pa_rt_memset(s->d_fail, 0, sizeof(int)) ||
        pa_k_bj_band_assemble(s->d_bm_src, s->d_bm_dst, s->d_bm_chunk_blk, s->d_bm_chunk_first, s->bm_nchunks, s->d_boff,
                              d_pv, d_band) ||
        /* new values can split a class of identical blocks: every block that read another one's records at the
         * create is compared with it again, on the assembled bands, and reads its own records if they differ
         * (sharing only shrinks here; blocks that became equal are found by a fresh create) */
        (s->share_members > 0 &&
         (pa_rt_memset(s->d_share_cnt, 0, 2 * sizeof(unsigned long long)) ||
          pa_k_bj_share_check(s->d_share_list, s->share_members, s->d_rep, s->d_nrows, s->d_bw, s->d_boff, d_band, s->d_off,
                              s->d_off2, s->d_off_read, s->d_off2_read, s->d_share_cnt))) ||
        pa_bj_factor_launch(s, s->d_slist, s->d_blist, s->d_boff, d_band, s->d_fail, &fail))
      rc = BJU_FAIL("factorising the diagonal blocks on the device failed: %s", pa_rt_error());
    *spd_fail = fail;
    if (!rc && s->share_members > 0) {
      unsigned long long cnt[2];
      if (pa_rt_d2h(cnt, s->d_share_cnt, sizeof(cnt))) rc = BJU_FAIL("%s", pa_rt_error());
      else {
        s->shared_blocks = (int)cnt[0]; s->shared_elems2 = (long long)cnt[1];
        /* The PAIR launch of bj_g4.hip serves a block from its partner's read offset: only while every block reads
         * what it read at the create.  A change of that is a change of what the apply launches: captured iteration
         * segments are taken anew. */
        const int intact = s->shared_blocks == s->share_members;
        if (intact != s->plan.pair_intact) { s->plan.pair_intact = intact; pa_bj_apply_epoch_bump(); }
      }
    }
  }
  if (!rc && fail == 0) {     /* the second layouts, from the new plain records */
    if (s->d_Lg4 && pa_bj_launch_g4(s)) rc = BJU_FAIL("k_bj_g4_setup failed");
    if (!rc && s->d_Lf2 && pa_bj_launch_pairs(s)) rc = BJU_FAIL("k_bj_pairs failed");
    if (!rc && (pa_rt_event_record(e1) || pa_rt_sync())) rc = BJU_FAIL("%s", pa_rt_error());
    if (!rc) s->upd_kernel_s = pa_rt_event_elapsed_s(e0, e1);
  }
  pa_rt_event_destroy(e0); pa_rt_event_destroy(e1);
  pa_rt_free(d_pv); pa_rt_free(d_band);
  return rc;
}

int preAlps_BlockJacobiUpdateValues(void) {
  pa_bj_t* s = pa_bj_state();
  const double t_all = pa_wtime();
  if (!s->created) return BJU_FAIL("preconditioner not created");
  const pa_operator_info_t* op = pa_operator_info();
  if (!op) return BJU_FAIL("operator not built: it was freed since preAlps_BlockJacobiCreate (free and create instead)");
  if (pa_operator_build_count() != s->op_build)
    return BJU_FAIL("the operator was built again since preAlps_BlockJacobiCreate: free and create instead");
  if (s->A_rowptr != op->A.rowPtr)
    return BJU_FAIL("the preconditioner was not created from the operator's own panel (preAlps_OperatorGetA): free and create instead");
  if (!s->dev_factor)
    return BJU_FAIL("the preconditioner was created with PREALPS_BJ_FACTOR=host, its records come from the host "
                    "Cholesky: free and create instead");
  int rc = 0, wrote = 0, spd_fail = 0;
  /* a coarse space on several processes is refreshed collectively below: a process whose own factor fails tells the
   * others before it returns, so that none waits for it there */
  const int co_ranks = s->co.on && s->co.multi;
  s->upd_copy_s = s->upd_kernel_s = 0.0;
  if (s->np - s->nd_blocks > 0) {
    rc = bj_ensure_band_map(s, op);
    if (rc) { if (co_ranks) pa_ranks_agree(1, NULL); return rc; }      /* (nothing of the factor has been touched) */
    rc = bj_refactor_bands(s, op, &wrote, &spd_fail);
    if (!rc && spd_fail > 0)
      rc = BJU_FAIL("diagonal block is not SPD (global row %d)",
                    pa_bj_fail_global_row(s->row_off, s->h_map_f, s->h_row0, s->h_nrows, s->np, spd_fail));
    if (rc && !wrote) { if (co_ranks) pa_ranks_agree(1, NULL); return rc; }
  }
  /* the blocks with the sparse factor: created again from the new panel, with the arguments of the create */
  if (!rc && s->nd_blocks > 0) {
    rc = pa_bj_nd_handoff("preAlps_BlockJacobiUpdateValues", &op->A, s->np, s->h_is_nd, s->nd_blocks, s->h_row0, s->h_nrows,
                          s->h_grow0, s->m, s->nd_bits, s->row_off);
    if (!rc) { s->nd_rebuilt = s->nd_blocks; s->factor_bytes = 2.0 * 8.0 * (double)s->lay.tot + pa_nd_factor_bytes(); }
  }
  /* the records hold the new values in part, or not even a factor: there is no old preconditioner to go back to */
  if (rc) { if (co_ranks) pa_ranks_agree(1, NULL); preAlps_BlockJacobiFree(); return rc; }
  ++s->updates;
  pa_bj_values_epoch_sync();
  if (co_ranks && pa_ranks_agree(0, NULL)) {
    if (pa_rt_sync()) { /* nothing more to report */ }
    pa_bj_coarse_release(&s->co);
    pa_bj_apply_epoch_bump();
    rc = BJU_FAIL("another process could not refresh its block factor: the coarse space was dropped, the refreshed block factor stays");
  } else if (s->co.on) rc = pa_bj_coarse_refresh(s, op);
  s->upd_total_s = pa_wtime() - t_all;
  return rc;
}

/* "bj_updates", "bj_band_map_*", "bj_update_*", the two addresses: preAlps_hip_get_stat; 0 = key known */
int pa_bj_update_stat(const char* key, double* value) {
  const pa_bj_t* s = pa_bj_state();
  const int on = s->created;
  if (!strcmp(key, "bj_updates")) *value = on ? s->updates : 0;
  else if (!strcmp(key, "bj_update_nd_rebuilt")) *value = on ? s->nd_rebuilt : 0;
  else if (!strcmp(key, "bj_band_map_builds")) *value = on ? s->bm_builds : 0;
  else if (!strcmp(key, "bj_band_map_entries")) *value = on && s->d_bm_src ? (double)s->bm_n : 0.0;
  else if (!strcmp(key, "bj_band_map_bytes")) *value = on && s->d_bm_src ? (double)s->bm_bytes : 0.0;
  else if (!strcmp(key, "bj_update_map_s")) *value = on ? s->upd_map_s : 0.0;
  else if (!strcmp(key, "bj_update_copy_s")) *value = on ? s->upd_copy_s : 0.0;
  else if (!strcmp(key, "bj_update_kernel_s")) *value = on ? s->upd_kernel_s : 0.0;
  else if (!strcmp(key, "bj_update_total_s")) *value = on ? s->upd_total_s : 0.0;
  /* the classes of identical blocks (bj_share.h): classes at the create, blocks that read another block's records
   * now (after a refresh: those that still do), bytes of the one-copy records that are read at all */
  else if (!strcmp(key, "bj_share_classes")) *value = on ? s->share_classes : 0;
  else if (!strcmp(key, "bj_shared_blocks")) *value = on ? s->shared_blocks : 0;
  else if (!strcmp(key, "bj_share_distinct_g4_bytes"))
    *value = on && s->d_Lg4 ? (s->g4_bits == 32 ? 4.0 : 8.0) * (double)(s->lay.tot2 - s->shared_elems2) : 0.0;
  else if (!strcmp(key, "bj_share_s")) *value = on ? s->share_s : 0.0;
  /* the pair tasks of the create (bj_share.h): wavefronts of the PAIR launch, blocks among them that have a partner */
  else if (!strcmp(key, "bj_pair_tasks")) *value = on ? s->pair_tasks : 0;
  else if (!strcmp(key, "bj_paired_blocks")) *value = on ? s->paired_blocks : 0;
  else if (!strcmp(key, "bj_records_address")) *value = on ? (double)(size_t)s->d_Lf : 0.0;
  else if (!strcmp(key, "bj_g4_address")) *value = on ? (double)(size_t)s->d_Lg4 : 0.0;
  else if (!strcmp(key, "bj_coarse_max_dofs")) *value = PA_COARSE_MAX_DOFS;
  else if (!strncmp(key, "bj_coarse_", 10)) {
    const pa_bj_coarse_t* co = &s->co;
    const int con = on && co->on;
    const char* sub = key + 10;
    if (!strcmp(sub, "dofs")) *value = con ? co->nc : 0;
    else if (!strcmp(sub, "vectors")) *value = con ? co->k : 0;
    else if (!strcmp(sub, "aggregates")) *value = con ? co->naggr : 0;
    else if (!strcmp(sub, "chunks")) *value = con ? co->nchunks : 0;
    else if (!strcmp(sub, "bytes")) *value = con ? co->bytes : 0.0;
    else if (!strcmp(sub, "setup_s")) *value = con ? co->setup_s : 0.0;
    else if (!strcmp(sub, "builds")) *value = con ? co->builds : 0;
    else if (!strcmp(sub, "applies")) *value = con ? (double)co->applies : 0.0;
    else if (!strcmp(sub, "einv_address")) *value = con ? (double)(size_t)co->d_Einv : 0.0;
    else return 1;
  }
  else return 1;
  return 0;
}
