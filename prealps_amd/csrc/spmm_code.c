/*
 * spmm_code.c -- codes the packed value array of a run plan: per workgroup block the distinct bit patterns, most
 * frequent first, and one 2-byte code per element (spmm_code.h).  Host arithmetic only.
 */
#include <stdlib.h>
#include <string.h>

#include "spmm_code.h"

void pa_spmm_code_free(pa_spmm_code_t* cd) {
  if (!cd) return;
  free(cd->code); free(cd->tab); free(cd->blk_tab_off);
  memset(cd, 0, sizeof(*cd));
}

#define CODE_MAX_ENTRIES 65536
#define CODE_HASH_BITS 17                       /* twice the entries a table may have */
#define CODE_HASH_SIZE ((size_t)1 << CODE_HASH_BITS)

typedef struct { uint64_t bits; uint32_t cnt; uint32_t idx; } code_entry_t;

/* most frequent first, ties by ascending bit pattern */
static int by_count(const void* a, const void* b) {
  const code_entry_t* x = (const code_entry_t*)a;
  const code_entry_t* y = (const code_entry_t*)b;
  if (x->cnt != y->cnt) return x->cnt > y->cnt ? -1 : 1;
  return x->bits < y->bits ? -1 : x->bits > y->bits;
}

int pa_spmm_code_build(const pa_spmm_pack_t* pk, const int* blk_slice, int nblk, const long long* sl_off,
                       const int* sl_row0, const int* sl_nrows, const int* blk_ext_off, int runs, int ts, int budget,
                       pa_spmm_code_t* cd) {
  memset(cd, 0, sizeof(*cd));
  if (!pk || !pk->meta || !pk->val || !runs || nblk < 0 || ts <= 0 || !blk_slice || !sl_off || !sl_row0 || !sl_nrows ||
      !blk_ext_off)
    return -2;
  /* the blocks are runs of slices behind each other, the slices whole steps of the pack */
  if (nblk > 0 && blk_slice[0] != 0) return -2;
  for (int b = 0; b < nblk; ++b) {
    const int s0 = blk_slice[b], s1 = blk_slice[b + 1];
    if (s1 <= s0 || sl_off[s0] % 64 || sl_off[s1] % 64 || sl_off[s1] < sl_off[s0] ||
        (size_t)(sl_off[s1] / 64) > pk->nsteps || blk_ext_off[b + 1] < blk_ext_off[b])
      return -2;
  }
  if (nblk > 0 && (size_t)(sl_off[blk_slice[nblk]] / 64) != pk->nsteps) return -2;

  size_t tab_cap = 4096;
  cd->code = (uint16_t*)malloc((pk->nval_alloc ? pk->nval_alloc : 1) * sizeof(uint16_t));
  cd->blk_tab_off = (int*)malloc(((size_t)nblk + 1) * sizeof(int));
  cd->tab = (double*)malloc(tab_cap * sizeof(double));
  /* one scratch block: the entries of a block in the order they were met, their ranks, a hash of them with a stamp
   * per place (the block that wrote it), so that nothing is cleared between blocks */
  code_entry_t* ent = (code_entry_t*)malloc(CODE_MAX_ENTRIES * (sizeof(code_entry_t) + sizeof(uint16_t)) +
                                            CODE_HASH_SIZE * 2 * sizeof(uint32_t));
  if (!cd->code || !cd->blk_tab_off || !cd->tab || !ent) { free(ent); pa_spmm_code_free(cd); return -1; }
  uint32_t* hidx = (uint32_t*)(ent + CODE_MAX_ENTRIES);
  uint32_t* hstamp = hidx + CODE_HASH_SIZE;
  uint16_t* rank = (uint16_t*)(hstamp + CODE_HASH_SIZE);
  memset(hstamp, 0, CODE_HASH_SIZE * sizeof(uint32_t));
  memset(cd->code, 0, (pk->nval_alloc ? pk->nval_alloc : 1) * sizeof(uint16_t));
  cd->ncode = pk->nval_alloc;
  cd->nblk = nblk;
  cd->coded_bytes = pk->packed_bytes;

  const uint64_t* vbits = (const uint64_t*)(const void*)pk->val;
  for (int b = 0; b < nblk; ++b) {
    cd->blk_tab_off[b] = (int)cd->ntab;
    const int s0 = blk_slice[b], s1 = blk_slice[b + 1];
    const size_t e0 = (size_t)pk->meta[4 * (size_t)(sl_off[s0] / 64) + 3], e1 = (size_t)pk->meta[4 * (size_t)(sl_off[s1] / 64) + 3];
    if (e1 < e0 || e1 > pk->nsteps + pk->nval) { free(ent); pa_spmm_code_free(cd); return -2; }
    const long long nown = (long long)sl_row0[s1 - 1] + sl_nrows[s1 - 1] - sl_row0[s0];
    const long long next = (long long)blk_ext_off[b + 1] - blk_ext_off[b];
    const long long stage = (nown + next + 2) * ts * 8;
    if (stage + 8 > budget || cd->ntab > 0x3fffffffu) continue;        /* raw: not even entry 0 fits (or the offsets would leave an int) */
    long long room = (budget - stage) / 8;                             /* entries the table may have */
    if (room > CODE_MAX_ENTRIES) room = CODE_MAX_ENTRIES;
    /* first pass: the distinct patterns in the order they are met; code[] holds that order for now */
    uint32_t n = 1;
    ent[0].bits = 0; ent[0].cnt = 0; ent[0].idx = 0;
    uint64_t last = 0; uint32_t last_idx = 0;
    int fits = 1;
    const uint32_t stamp = (uint32_t)b + 1;
    for (size_t i = e0; i < e1; ++i) {
      const uint64_t v = vbits[i];
      uint32_t idx = 0;
      if (v == last) idx = last_idx;
      else if (v == 0) idx = 0;
      else {
        size_t h = (size_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - CODE_HASH_BITS));
        for (;;) {
          if (hstamp[h] != stamp) {
            if ((long long)n >= room) { fits = 0; break; }
            hstamp[h] = stamp; hidx[h] = n;
            ent[n].bits = v; ent[n].cnt = 0; ent[n].idx = n;
            idx = n++;
            break;
          }
          if (ent[hidx[h]].bits == v) { idx = hidx[h]; break; }
          h = (h + 1) & (CODE_HASH_SIZE - 1);
        }
        if (!fits) break;
      }
      last = v; last_idx = idx;
      ++ent[idx].cnt;
      cd->code[i] = (uint16_t)idx;
    }
    if (!fits) {                                                       /* raw: the codes written so far go */
      memset(cd->code + e0, 0, (e1 - e0) * sizeof(uint16_t));
      continue;
    }
    if (cd->ntab + n > tab_cap) {
      while (cd->ntab + n > tab_cap) tab_cap *= 2;
      double* t = (double*)malloc(tab_cap * sizeof(double));
      if (!t) { free(ent); pa_spmm_code_free(cd); return -1; }
      memcpy(t, cd->tab, cd->ntab * sizeof(double));
      free(cd->tab);
      cd->tab = t;
    }
    if (n > 2) qsort(ent + 1, n - 1, sizeof(code_entry_t), by_count);
    for (uint32_t c = 0; c < n; ++c) {
      rank[ent[c].idx] = (uint16_t)c;
      memcpy(cd->tab + cd->ntab + c, &ent[c].bits, sizeof(double));
    }
    for (size_t i = e0; i < e1; ++i) cd->code[i] = rank[cd->code[i]];
    cd->ntab += n;
    ++cd->ncoded;
    cd->coded_elems += e1 - e0;
    if ((int)(stage + 8 * (long long)n) > cd->lds_bytes) cd->lds_bytes = (int)(stage + 8 * (long long)n);
  }
  cd->blk_tab_off[nblk] = (int)cd->ntab;
  cd->coded_bytes = pk->packed_bytes - 6.0 * (double)cd->coded_elems + 8.0 * (double)cd->ntab;
  free(ent);
  return 0;
}
