/*
 * bj_build.h -- the host work of creating the band block-Jacobi preconditioner (bj_build.c): per block the
 * factor order (reverse Cuthill-McKee, or the given order where that is no wider), the band in row-major or
 * entry-list form, the host band Cholesky and the sweep records of a host-factored block; and, once per create,
 * the layout table every stage and the later refresh read.  Pure host arithmetic on libc + OpenMP: no device
 * call, no environment, no globals, so it runs under a host sanitizer and in tests without a GPU
 * (tests/c/bj_build_check.c).  The kernels' constants and the switches arrive as fields of the input structs;
 * block_jacobi.c fills them, uploads the results and launches the kernels.
 */
#ifndef PA_BJ_BUILD_H
#define PA_BJ_BUILD_H

#include <stddef.h>

#include "bj_band_map.h"   /* pa_bj_band_len: the length of a block's assembled band */
#include "pa_device.h"     /* pa_bj_wide_window: the one rule shared with the kernels */

enum { PA_BJ_OK = 0, PA_BJ_NOMEM = -1, PA_BJ_NOT_SPD = -2, PA_BJ_BANDWIDTH = -3 };

/* Doubles of one sweep record of a block with bandwidth w.  Narrow bands (one wavefront per block): w + 1
 * rounded up to even, [L(j+1..j+w, j) / L(j,j) | 0].  Bands above wide_from (one workgroup per block): the
 * window W = pa_bj_wide_window(w) >= w + 64, in window-slot order, the value for target row i at i mod W. */
static inline int pa_bj_reclen(int w, int wide_from) { return w > wide_from ? pa_bj_wide_window(w) : ((w + 2) & ~1); }

/* ---- per block ------------------------------------------------------------------------------------------- */
/* What the blocks are built from; every pointer is borrowed. */
typedef struct {
  int np, m;                  /* blocks and rows of the panel */
  const int* rowPtr;          /* the panel: local rows, global column ids */
  const int* colInd;
  const double* val;
  const int* grow;            /* np + 1: global row (= column) of every block's first row, and the end */
  int row_off;                /* global row of the panel's first row (= grow[0]) */
  int nd_mode, nd_rows;       /* sparse factor instead of a band: 0 never, 1 for blocks of at least nd_rows rows whose
                                 band exceeds 256, 2 for every block of at least nd_rows rows */
  int dev_factor;             /* 1: the device factors the bands, 0: pa_bj_band_cholesky does, here */
  int dev_wmax;               /* dev_factor: bands up to dev_wmax are assembled row-major, wider ones as entry lists */
  int threads;                /* OpenMP threads (< 1: one) */
} pa_bj_build_in_t;

/* The blocks on the host; owns its arrays. */
typedef struct {
  int np, m;
  int* row0; int* nrows;      /* np: first local row and rows of every block */
  int* bw;                    /* np: bandwidth in factor order */
  char* is_nd;                /* np: 1 = the block gets the sparse factor and no band */
  int* map_f; int* map_b;     /* m: block-local row at forward / backward step j of its block */
  double* invd_f; double* invd_b;   /* m: 1 / L(j,j) in step order (pa_bj_layout_slab fills them) */
  double** bands;             /* np: row-major band, band[i*(w+1) + d] = A(new i, new i-d) (the factor when !dev_factor) */
  long long** coo_off; double** coo_val; size_t* coo_n;   /* np: the entries of a band above dev_wmax, offset
                                 d*b + i (diagonal-major) in the block's band and value */
  int fail_row;               /* after PA_BJ_NOT_SPD: global row of a non-positive pivot, else -1 */
  int nomem_block;            /* after PA_BJ_NOMEM: a block that could not allocate, -1: the arrays of the panel */
} pa_bj_build_t;

/* One pass over the blocks (OpenMP, in->threads): order, bandwidth, the sparse-factor decision, band assembly,
 * host band Cholesky when !in->dev_factor.  Returns PA_BJ_OK, PA_BJ_NOMEM or PA_BJ_NOT_SPD; after a failure the
 * build is empty but for fail_row / nomem_block. */
int pa_bj_build_blocks(const pa_bj_build_in_t* in, pa_bj_build_t* B);
/* Release a build in any state (zeroed, failed, bands partly handed on and set to NULL); leaves it empty. */
void pa_bj_build_free(pa_bj_build_t* B);

/* In-place band Cholesky (band[i*(w+1) + d] = L(i, i-d)); returns the first row whose pivot is not positive
 * (the factor carries NaN from there on), -1 if none. */
int pa_bj_band_cholesky(double* band, int b, int w);

/* Steps [j0, j0 + 256) of block x from its factored band B->bands[x] into the forward / backward records f / g
 * (the block's records, zeroed by the caller, pa_bj_reclen(w, wide_from) doubles per step) and B->invd_f / invd_b:
 *   invd_f[j] = 1 / L(j,j),  f: L(j+d, j) * invd_f[j],  d = 1..w, at slot d-1 (narrow) or (j+d) mod W (wide)
 *   invd_b[j] = 1 / L(jr,jr), g: L(jr, jr-d) * invd_b[j] at the same slot, jr = b-1-j. */
void pa_bj_layout_slab(pa_bj_build_t* B, int wide_from, int x, int j0, double* f, double* g);

/* ---- the layout, once per create ----------------------------------------------------------------------- */
typedef struct {
  int np;
  const int* nrows; const int* bw; const char* is_nd;   /* np each, borrowed */
  int factor_wmax;            /* widest band of k_bj_factor (pa_bj_factor_wmax) */
  int max_R;                  /* register sets per lane of the one-wavefront kernels (pa_bj_max_R) */
  int g4_max_band, g4_max_rows;   /* what bj_g4.hip takes */
  int dev_factor;
  int wide_from;              /* PREALPS_BJ_WIDE_FROM; negative: absent */
  int want_g4, want_pairs;
} pa_bj_layout_in_t;

#define PA_BJ_MAX_CLASSES 16

/* Every size, offset and list the stages of the create and preAlps_BlockJacobiUpdateValues need; owns its arrays. */
typedef struct {
  int np;
  int wide_from;              /* bands above it get one workgroup per block: factor_wmax below 1024 blocks, else
                                 64 * max_R - 64; the override clamped into that range */
  long long* off;             /* np + 1: record offset of every block, doubles (sparse blocks: no records) */
  size_t tot;                 /* off[np] */
  long long maxrec;           /* longest narrow record */
  size_t pad;                 /* slack behind the records: 256 + 8 * maxrec doubles */
  int ndev, nnd;              /* blocks the device factors / blocks with the sparse factor */
  int max_bw;                 /* widest band, sparse blocks included */
  int bad_bw;                 /* after PA_BJ_BANDWIDTH: the band that was refused */
  /* classes by register sets: a narrow block needs R = ceil((w + 64) / 64) per lane, a wide one is in class
   * -(register sets per lane of k_bj_wide); sparse blocks are in none.  Lists in block order. */
  int nclass;
  int class_R[PA_BJ_MAX_CLASSES], class_count[PA_BJ_MAX_CLASSES], class_wmax[PA_BJ_MAX_CLASSES], class_bmax[PA_BJ_MAX_CLASSES];
  int* class_list[PA_BJ_MAX_CLASSES];
  /* second layouts of the narrow classes: one-copy records (bj_g4.hip) / paired records (k_bj_pairs) */
  int class_g4[PA_BJ_MAX_CLASSES], class_pairs[PA_BJ_MAX_CLASSES], any_g4, any_pairs;
  long long* off2;            /* np + 1: element offset of a narrow block's second record, 8 ceil(b/8) (w+4) each; */
  long long tot2;             /* all zero unless any_g4 or any_pairs */
  /* the assembled bands and the launch lists of the two factorisation kernels */
  long long* boff;            /* np + 1: offset of every block's band (pa_bj_band_len) */
  size_t btot;
  int* slist; int ns, wsmall; /* bands up to factor_wmax: k_bj_factor */
  int* blist; int nbig, wbig; /* wider: k_bj_factor_big */
} pa_bj_layout_t;

/* Returns PA_BJ_OK, PA_BJ_NOMEM, or PA_BJ_BANDWIDTH when the window of a band exceeds 4096 (bad_bw, and the
 * reason in err, errlen bytes, may be NULL).  The layout is empty after a failure, but for bad_bw. */
int pa_bj_layout_build(const pa_bj_layout_in_t* in, pa_bj_layout_t* L, char* err, size_t errlen);
/* Release a layout in any state; leaves it empty. */
void pa_bj_layout_free(pa_bj_layout_t* L);

#endif
