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

/* A coarse space on the host; owns its arrays. */
typedef struct {
  int m, k, naggr, nc, nchunks;
  double* zv;                 /* m x k */
  int* ch_row0; int* ch_nrows; int* ch_aggr;   /* nchunks each */
  int* agg_ptr;               /* naggr + 1 */
  int* agg_chunk;             /* nchunks: chunk ids, aggregate after aggregate, ascending inside one */
  double* E;                  /* nc x nc */
  double* Einv;               /* nc x nc, symmetric in bits */
  int bad_aggr, bad_vec;      /* after PA_COARSE_SINGULAR (and for an empty / out-of-range aggregate: bad_aggr) */
} pa_coarse_t;

enum { PA_COARSE_OK = 0, PA_COARSE_NOMEM = -1, PA_COARSE_CAP = -2, PA_COARSE_AGGR = -3, PA_COARSE_SINGULAR = -4,
       PA_COARSE_ARG = -5 };

/* Builds *out (zeroed on entry by the call) and returns PA_COARSE_OK, or a code above with the reason in err
 * (errlen bytes, may be NULL) and *out empty again: nothing is left half built.  A pivot <= nc * eps * max diag
 * E is PA_COARSE_SINGULAR; the message names the aggregate and the vector. */
int pa_coarse_build(const pa_coarse_in_t* in, pa_coarse_t* out, char* err, size_t errlen);
void pa_coarse_free(pa_coarse_t* c);

/* k-way partition of a graph (0-based CSR, diagonal stored), the signature of preAlps_hip_partition_kway */
typedef int (*pa_coarse_kway_fn)(int n, const int* rowPtr, const int* colInd, int nparts, int* part);
/* The aggregates when the caller gives none (part_aggregate: nparts ints, written): one per part when
 * nparts * k <= max_dofs (<= 0: PA_COARSE_MAX_DOFS), otherwise floor(max_dofs / k) aggregates from kway on the
 * quotient graph of the parts -- an edge between parts p and q when some a_ij joins them, diagonal stored --
 * numbered without gaps, so *naggr may come out smaller.  in->part_aggregate, naggr and Vp are not read. */
int pa_coarse_default_aggregates(const pa_coarse_in_t* in, pa_coarse_kway_fn kway, int* part_aggregate, int* naggr,
                                 char* err, size_t errlen);

#endif
