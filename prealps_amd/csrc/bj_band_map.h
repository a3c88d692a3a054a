/*
 * bj_band_map.h -- where the values of the assembled bands of the block-Jacobi preconditioner come from
 * (bj_band_map.c).  Pure host arithmetic on libc: no device call, no environment, no globals, so it runs
 * under a host sanitizer and in tests without a GPU.  block_jacobi.c uploads the result and
 * bj_refactor.hip applies it (preAlps_BlockJacobiUpdateValues).
 */
#ifndef PA_BJ_BAND_MAP_H
#define PA_BJ_BAND_MAP_H

#include <stddef.h>
#include <stdint.h>

/* What a map is cut from; every pointer is borrowed. */
typedef struct {
  int np;                /* blocks of the panel */
  const int* rowPtr;     /* the panel: local rows, global column ids */
  const int* colInd;
  const int* row0;       /* np: first local row of every block */
  const int* nrows;      /* np */
  const int* grow0;      /* np: global row (= column) of the block's first row */
  const int* bw;         /* np: bandwidth of the block in factor order */
  const int* order;      /* order[row0[q] + j] = block-local row at factor position j (the map_f of the create) */
  const char* is_nd;     /* np: 1 = the block has the sparse factor and no band */
  int wmax;              /* bands up to wmax are row-major, wider ones diagonal-major */
  int chunk;             /* most entries of one chunk (<= 0: 1024) */
} pa_bj_band_map_in_t;

/* One entry per panel entry inside a band block's diagonal block, on or below the diagonal in factor order
 * (A(ni, nj) with nj <= ni the factor positions of its row and column), blocks, rows and entries in panel
 * order, so src ascends:
 *   band[boff[q] + dst[e]] = val[src[e]]
 * with dst[e] = ni * (w + 1) + ni - nj (row-major, w <= wmax) or (ni - nj) * b + ni (diagonal-major), as the
 * host assembly of the create places it; every other entry of the zeroed band array stays zero.  Where a row
 * holds a column twice only the last entry is in the map (the one a host assembly that overwrites keeps), so
 * no two entries share a destination.  Chunks never cross a block: chunk c is the entries
 * [chunk_first[c], chunk_first[c + 1]) of block chunk_blk[c]. */
typedef struct {
  uint32_t* src;           /* n: index into the panel's val */
  uint32_t* dst;           /* n: offset inside the block's band */
  size_t n;
  int* chunk_blk;          /* nchunks */
  uint32_t* chunk_first;   /* nchunks + 1 */
  size_t nchunks;
  long long* boff;         /* np + 1: offset of every block's band of nrows * (bw + 1) doubles (sparse blocks: none) */
  int bad_block;           /* after -2 / -3: the block that was refused */
} pa_bj_band_map_t;

/* The one statement of a band's length: nrows * (bw + 1) doubles, none for a sparse-factored block (bj_build.c
 * lays out the bands of the create by it, bj_band_map.c those of the refresh). */
static inline long long pa_bj_band_len(int nrows, int bw, int is_nd) { return is_nd ? 0 : (long long)nrows * ((long long)bw + 1); }

/* Returns 0, -1 when out of memory, -2 when a block's band has 2^32 entries or more, -3 when an entry of a
 * block lies outside its band (bw is not the bandwidth of order); bad_block names the block.  The map is empty
 * after a failure. */
int pa_bj_band_map_build(const pa_bj_band_map_in_t* in, pa_bj_band_map_t* map);
/* Release a map in any state; leaves it empty. */
void pa_bj_band_map_free(pa_bj_band_map_t* map);
/* device bytes of a map: 8 per entry + the chunk list */
static inline size_t pa_bj_band_map_bytes(const pa_bj_band_map_t* map) {
  return map->n * 2 * sizeof(uint32_t) + map->nchunks * sizeof(int) + (map->nchunks + 1) * sizeof(uint32_t);
}

#endif
