/*
 * mtx_read.h -- the MatrixMarket reader of preAlps_OperatorBuild on the host (mtx_read.c): a file name in, the
 * matrix in CSR out.  Pure host code on libc + OpenMP: no device call, no environment, no globals, so it runs
 * under a host sanitizer and in tests without a GPU.  operator.c passes its thread count and reports `err`.
 */
#ifndef PA_MTX_READ_H
#define PA_MTX_READ_H

#include <stddef.h>

/* A matrix read from a file; owns its arrays.  Columns ascending in every row, repeated entries summed. */
typedef struct {
  int N;
  int* rowPtr;      /* N + 1 */
  int* colInd;
  double* val;
} pa_mtx_t;

enum { PA_MTX_OK = 0, PA_MTX_NOMEM = -1, PA_MTX_OPEN = -2, PA_MTX_FORMAT = -3, PA_MTX_ENTRY = -4 };

/* Reads `file` with up to `threads` OpenMP threads (< 1: one); trace != 0 prints the "[setup]" lines of the
 * stages to stderr.  Returns PA_MTX_OK, or a code above with the reason in err (errlen bytes, may be NULL) and
 * *out empty again. */
int pa_mtx_read(const char* file, int threads, int trace, pa_mtx_t* out, char* err, size_t errlen);
void pa_mtx_free(pa_mtx_t* m);

#endif
