/*
 * bj_share.h -- which diagonal blocks of the band block-Jacobi preconditioner are the same block (bj_share.c).
 * On a matrix assembled from one element matrix most diagonal blocks repeat: same rows, same bandwidth, the same
 * band in factor order, bit for bit.  Identical bands get identical factors and identical sweep records, so the
 * apply may read one block's records for all of them (block_jacobi.c: the read offsets) and the record stream comes
 * out of the L2 instead of HBM.  Here only the classes are found.  Pure host arithmetic on libc + OpenMP: no device
 * call, no environment, no globals (tests/c/bj_share_check.c runs it under the host sanitizers).
 */
#ifndef PA_BJ_SHARE_H
#define PA_BJ_SHARE_H

#include <stddef.h>

/* What the classes are found from; every pointer is borrowed. */
typedef struct {
  int np;
  const int* nrows; const int* bw;     /* np each */
  const char* eligible;                /* np: 1 = the block may share (a narrow block whose band is assembled row-major) */
  double* const* bands;                /* np: row-major band of nrows * (bw + 1) doubles; read for eligible blocks only */
  int threads;                         /* OpenMP threads (< 1: one) */
  unsigned long long hash_mask;        /* and-ed onto every hash: ~0 in use; tests pass fewer bits (0: every eligible
                                          block is a candidate of every other) to see that a hash decides nothing */
} pa_bj_share_in_t;

/* rep[p] (np ints, the caller's) = the lowest-numbered eligible block with the same nrows, bw and band bytes as p, or
 * p itself (always for a block that is not eligible).  Equality is that of the bytes (memcmp): -0.0 is not +0.0, a
 * NaN equals its own bit pattern only.  The hash of a band only picks the candidates; every match is verified
 * against its representative.  *nclass = blocks with rep[p] == p.  Returns 0, or -1 out of host memory (rep[p] = p
 * for every block then: nothing shares). */
int pa_bj_share_classes(const pa_bj_share_in_t* in, int* rep, int* nclass);

/* The pair tasks of one launch list (bj_g4.hip, the PAIR launch: two blocks of one class in one wavefront, the record
 * read once for both).  list[0 .. count) = the blocks of the launch in launch order, rep[] as above (np entries).
 * tasks[2 k], tasks[2 k + 1] = positions (i0, i1) INTO list of the two members of task k: rep[list[i0]] ==
 * rep[list[i1]], i0 < i1; i1 = -1 for a block without a partner (the last of an odd class, a class of one, a block
 * that is not eligible and so is its own class).  Every position appears in exactly one task; the pairs of a class are
 * formed in list order (its first with its second, its third with its fourth, ...) and the tasks are ordered by i0.
 * One pass over the list with one slot per block, no hash: the same list gives the same tasks.  Blocks with one rep
 * have the same rows and bandwidth by construction; the function asserts it.  tasks: 2 * count ints, the caller's.
 * *ntasks = tasks, *paired = blocks that have a partner (2 x the tasks with i1 >= 0).  Returns 0, or -1 out of host
 * memory (*ntasks = *paired = 0 then). */
int pa_bj_pair_tasks(int np, const int* list, int count, const int* rep, const int* nrows, const int* bw, int* tasks,
                     int* ntasks, int* paired);

#endif
