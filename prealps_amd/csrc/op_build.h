/*
 * op_build.h -- the shard of one process on the host (op_build.c): the matrix (or the raw rows of one panel), a
 * partition and the place of the process in its group in; the ordering, the scaling vector, the row panel with
 * its halo slots and the send lists out.  Pure host arithmetic on libc + OpenMP: no device call, no
 * environment, no globals, no process group, so it runs under a host sanitizer and in tests without a GPU.
 * operator.c adopts the finished shard and uploads what the device needs.
 *
 *   Ordering: rows grouped part by part, original order inside a part; perm[new] = old, iperm[old] = new,
 * rowPos[p] = first new row of part p.  Process g of `size` owns parts [g nparts / size, (g + 1) nparts / size).
 *   Scaling (SymRACScaling): d_i = 1 / sqrt(max_j |a_ij|); the panel holds d[old row] * a * d[old column].
 *   Panel: rows [row_off, row_off + m) of the permuted, scaled matrix, columns in the new numbering, ascending.
 * Halo slots: the distinct columns outside the own range, ascending (halo_cols), hence grouped by owner;
 * lcol = column - row_off for an own column, m + slot for a halo column.
 *   Send lists: process g receives from us the rows of ours that occur as columns in ITS rows, ascending --
 * which is how g numbers its halo slots.
 */
#ifndef PA_OP_BUILD_H
#define PA_OP_BUILD_H

#include <stddef.h>

/* What a shard is built from; every pointer is borrowed. */
typedef struct {
  int N;                  /* global rows */
  const int* rowPtr;      /* the whole matrix, original numbering (pa_op_panel with whole = 0: the raw rows of */
  const int* colInd;      /* this process's panel only, row i of the panel first, columns still original) */
  const double* val;
  int nparts;
  const int* part;        /* N part ids, or NULL: contiguous row blocks */
  int scale;              /* != 0: SymRACScaling */
  int rank, size;         /* this process in its group */
  int threads;            /* OpenMP threads (< 1: one) */
  int trace;              /* != 0: the "[setup]" lines of the stages on stderr */
} pa_op_in_t;

/* The shard; owns its arrays.  Filled stage by stage: pa_op_order -> pa_op_panel -> pa_op_peers_whole or
 * pa_op_finish_peers. */
typedef struct {
  int N, nparts;
  int* rowPos;            /* nparts + 1 */
  int* perm;              /* N */
  int* iperm;             /* N: scratch of the build, not part of the operator */
  double* d;              /* N, or NULL: not scaled */
  int part0, part1, row_off, m, lnnz, halo;
  int* rowPtr;            /* m + 1 */
  int* colInd;            /* lnnz: new global column ids */
  double* val;
  int* src;               /* lnnz: index into the input's val of every panel entry; NULL unless asked */
  int* lcol;              /* lnnz + 8 (the last 8 are zero: spare entries the plan builders may read) */
  int* halo_cols;         /* halo: new global row of every halo slot, ascending */
  int* recv_by_proc;      /* size: halo slots owned by every process */
  int npeers, nsend;
  int* peers;             /* npeers process ids (room for size) */
  int* send_rows;         /* per peer */
  int* recv_rows;
  int* send_idx;          /* nsend: local rows packed for the peers, peer after peer */
} pa_op_shard_t;

enum { PA_OP_OK = 0, PA_OP_NOMEM = -1, PA_OP_DIAG = -2, PA_OP_SCALE = -3, PA_OP_PART = -4, PA_OP_DUP = -5,
       PA_OP_SIZE = -6 };

/* Every builder returns PA_OP_OK, or a code above with the reason in err (errlen bytes, may be NULL) and *sh
 * empty again (as pa_op_shard_free leaves it): nothing is left half built. */
void pa_op_shard_free(pa_op_shard_t* sh);

int pa_op_owner_of_part(int p, int nparts, int size);
int pa_op_part_of_row(const int* rowPos, int nparts, int row);   /* rowPos[p] <= row < rowPos[p + 1] */

/* d[i] = 1 / sqrt(max_k |val[k]|) over row i, the one statement of the scaling vector; returns 1 when a row
 * holds no nonzero value (its d is 0.0), else 0. */
int pa_op_scaling(int N, const int* rowPtr, const double* val, int threads, double* d);

/* The one statement of a panel value: d[old row] * v * d[old column], in that order (d NULL: v). */
static inline double pa_op_panel_value(const double* d, int old_row, double v, int old_col) {
  return d ? d[old_row] * v * d[old_col] : v;
}
/* out[e] = the panel value of entry e from new values in the input's order (val[src[e]]), for every entry of
 * the m rows of a panel built with keep_src */
void pa_op_panel_values(int m, int row_off, const int* rowPtr, const int* colInd, const int* src, const int* perm,
                        const double* d, const double* val, int threads, double* out);

/* *sh zeroed on entry by the call.  Checks that every row holds its diagonal entry (the message names the
 * lowest row that does not), forms d when in->scale, and the ordering: N, nparts, rowPos, perm, iperm, d. */
int pa_op_order(const pa_op_in_t* in, pa_op_shard_t* sh, char* err, size_t errlen);

/* The panel of process in->rank from an ordered shard: row i of the panel is row (whole ? perm[row_off + i] : i)
 * of in->rowPtr / colInd / val.  keep_src: also sh->src. */
int pa_op_panel(const pa_op_in_t* in, pa_op_shard_t* sh, int whole, int keep_src, char* err, size_t errlen);

/* peers / send_rows / recv_rows / nsend / send_idx from need-lists: asked = for every process g (in rank
 * order) the local rows of ours it reads, asked_cnt[g] of them, ascending.  Takes `asked` over (free()d on
 * failure too). */
int pa_op_finish_peers(pa_op_shard_t* sh, int size, int* asked, const int* asked_cnt, char* err, size_t errlen);

/* The same from the whole matrix (in->rowPtr / colInd: every process holds it), without communication. */
int pa_op_peers_whole(const pa_op_in_t* in, pa_op_shard_t* sh, char* err, size_t errlen);

/* The inverse of send_idx.  off (m + 2 ints, zero on entry; m + 1 used on return), slot (nsend ints): row r is
 * packed into the send-buffer slots slot[off[r] .. off[r + 1]), ascending (a row goes to every neighbour that
 * reads it). */
void pa_op_inverse_send_list(int m, int nsend, const int* send_idx, int* off, int* slot);

#endif
