/*
 * coarse_space.h -- the coarse space of the two-level block-Jacobi preconditioner on the host
 * (coarse_space.c): panel CSR, parts, aggregates and k vectors in; Z (as zv), the chunk lists of the device
 * kernels, E = Z^T A Z and its explicit inverse out.  Pure host arithmetic on libc + OpenMP: no device call,
 * no environment, no globals, so it runs under a host sanitizer and in tests without a GPU.
 * block_jacobi.c uploads the result.
 *
 *   Z: row i of part p in aggregate g = part_aggregate[p] has its k values in columns g*k .. g*k + k - 1, so Z
 * is stored as the m x k row-major array zv and nc = naggr * k.
 *   Chunks: every part is cut into chunks of at most PA_COARSE_CHUNK consecutive rows (first row, row count,
 * aggregate); agg_ptr / agg_chunk list each aggregate's chunks in ascending order.
 *   E(g*k + a, h*k + b) = sum_ij zv[i][a] a_ij zv[j][b] over the rows i of aggregate g and the columns j of
 * aggregate h.  A thread owns whole aggregates' rows and adds in row order: the bits do not depend on the
 * number of threads.  Einv = L^-T L^-1 from the fp64 Cholesky factor E = L L^T, lower triangle copied onto the
 * upper.
 *   Several processes: the build has two stages.  (a) pa_coarse_share: a rank's share from its own rows of the
 * panel -- zv and the chunk lists of its rows, agg_ptr over ALL aggregates (an aggregate without a chunk here has
 * an empty list), the coarse rows it needs, and E_r, the sum over its rows i alone (column j, a global id, goes to
 * the aggregate of its part).  The E_r of all ranks add up to E; an entry whose rows lie on one rank is that
 * rank's value plus zeros.  (b) pa_coarse_invert: E -> Einv, the same bits wherever it runs on the same E.
 * pa_coarse_build is (a) on all rows, then (b).
 */
#ifndef PA_COARSE_SPACE_H
#define PA_COARSE_SPACE_H

#include <stddef.h>

#define PA_COARSE_MAX_DOFS 1536   /* cap on nc: 18.9 MB of Einv, about nc^3 host flops */
#define PA_COARSE_CHUNK    1024   /* rows of a chunk at most */
#define PA_COARSE_MAX_VECS 8

/* What a coarse space is built from; every pointer is borrowed. */
typedef struct {
  int m;                      /* rows of the panel (one process: all of them) */
  int nparts;
  const int* rowPtr;          /* m + 1 */
  const int* lcol;            /* local column ids; entries with a column >= m are skipped */
  const double* val;
  const int* rowPos;          /* nparts + 1: first local row of every part, rowPos[0] = 0, rowPos[nparts] = m */
  const int* part_aggregate;  /* nparts values in [0, naggr), every aggregate non-empty */
  int naggr;
  int k;                      /* vectors, 1 .. PA_COARSE_MAX_VECS */
  const double* Vp;           /* m x k row major, internal space */
  int max_dofs;               /* cap on naggr * k; <= 0: PA_COARSE_MAX_DOFS */
  int threads;                /* OpenMP threads; <= 0: the runtime's default */
} pa_coarse_in_t;

/* What a rank's share is built from (stage (a)); every pointer is borrowed. */
typedef struct {
  int m;                      /* the rank's rows */
  int row_off;                /* global id of its first row */
  int nparts;                 /* parts of all ranks */
  int part0, np_loc;          /* the rank's parts: rowPos[part0] = row_off, rowPos[part0 + np_loc] = row_off + m */
  const int* rowPtr;          /* m + 1 */
  const int* gcol;            /* global column ids; an entry outside 0 .. rowPos[nparts] - 1 is skipped */
  const double* val;
  const int* rowPos;          /* nparts + 1, global */
  const int* part_aggregate;  /* nparts values in [0, naggr), every aggregate non-empty; may span ranks */
  int naggr;
  int k;
  const double* Vp;           /* row j (global id) at Vp + j * k: read for the rank's rows and the columns its panel touches */
  int max_dofs;
  int threads;
} pa_coarse_share_in_t;

/* A coarse space on the host; owns its arrays. */
typedef struct {
  int m, k, naggr, nc, nchunks;
  int row_off;                /* global id of local row 0 (0 after pa_coarse_build) */
  double* zv;                 /* m x k */
  int* ch_row0; int* ch_nrows; int* ch_aggr;   /* nchunks each; ch_row0 counts from the share's first row */
  int* agg_ptr;               /* naggr + 1 */
  int* agg_chunk;             /* nchunks: chunk ids, aggregate after aggregate, ascending inside one */
  int nrows; int* rows;       /* the coarse rows g*k .. g*k + k - 1 of the aggregates g with a chunk here, ascending */
  double* E;                  /* nc x nc; after pa_coarse_share: the share's E_r */
  double* Einv;               /* nc x nc, symmetric in bits (after pa_coarse_invert) */
  int bad_aggr, bad_vec;      /* after PA_COARSE_SINGULAR (and for an empty / out-of-range aggregate: bad_aggr) */
} pa_coarse_t;

enum { PA_COARSE_OK = 0, PA_COARSE_NOMEM = -1, PA_COARSE_CAP = -2, PA_COARSE_AGGR = -3, PA_COARSE_SINGULAR = -4,
       PA_COARSE_ARG = -5 };

/* Builds *out (zeroed on entry by the call) and returns PA_COARSE_OK, or a code above with the reason in err
 * (errlen bytes, may be NULL) and *out empty again: nothing is left half built.  A pivot <= nc * eps * max diag
 * E is PA_COARSE_SINGULAR; the message names the aggregate and the vector. */
int pa_coarse_build(const pa_coarse_in_t* in, pa_coarse_t* out, char* err, size_t errlen);
void pa_coarse_free(pa_coarse_t* c);
/* Stage (a): *out as above with E = E_r and Einv allocated but not formed; the refusals of pa_coarse_build but the
 * singular one.  The rows of E_r are added in the order of pa_coarse_build: rows of an aggregate in chunk-list
 * order, the entries of a row in order. */
int pa_coarse_share(const pa_coarse_share_in_t* in, pa_coarse_t* out, char* err, size_t errlen);
/* Stage (b): c->Einv from c->E (the caller has summed the shares into it); PA_COARSE_SINGULAR frees *c, names
 * aggregate and vector in err and leaves them in bad_aggr / bad_vec.  threads <= 0: the runtime's default. */
int pa_coarse_invert(pa_coarse_t* c, int threads, char* err, size_t errlen);

/* k-way partition of a graph (0-based CSR, diagonal stored), the signature of preAlps_hip_partition_kway */
typedef int (*pa_coarse_kway_fn)(int n, const int* rowPtr, const int* colInd, int nparts, int* part);
/* The aggregates when the caller gives none (part_aggregate: nparts ints, written): one per part when
 * nparts * k <= max_dofs (<= 0: PA_COARSE_MAX_DOFS), otherwise floor(max_dofs / k) aggregates from kway on the
 * quotient graph of the parts -- an edge between parts p and q when some a_ij joins them, diagonal stored --
 * numbered without gaps, so *naggr may come out smaller.  in->part_aggregate, naggr and Vp are not read. */
int pa_coarse_default_aggregates(const pa_coarse_in_t* in, pa_coarse_kway_fn kway, int* part_aggregate, int* naggr,
                                 char* err, size_t errlen);

/* The same for a rank of several (in->part_aggregate, naggr and Vp are not read): local_aggregate[q] in
 * [0, *naggr_loc) for the rank's part part0 + q.  One per part when nparts * k of ALL ranks fits the cap; otherwise
 * pa_coarse_default_aggregates on the quotient graph of the rank's own parts -- edges to other ranks' parts dropped
 * -- for max(1, floor(floor(cap / k) * np_loc / nparts)) aggregates.  The caller numbers them rank after rank, so
 * that no default aggregate spans ranks.  A rank without parts gets none. */
int pa_coarse_default_aggregates_share(const pa_coarse_share_in_t* in, pa_coarse_kway_fn kway, int* local_aggregate,
                                       int* naggr_loc, char* err, size_t errlen);

#endif
