/* Stand-alone run of prealps_amd/csrc/mtx_read.c (tests/test_mtx_read_unit_cpu.py).
 * usage: mtx_read_check <file.mtx> <threads>
 * Prints "N <n>", then rowPtr, colInd and val (%.17g), one array per line as "name count values..."; a file the
 * reader refuses prints "error <code> <message>" and "empty <0|1>" (1: the result came back empty). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mtx_read.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <file.mtx> <threads>\n", argv[0]); return 2; }
  pa_mtx_t A, zero;
  char err[600] = "";
  memset(&A, 0x5a, sizeof(A));   /* (the reader zeroes it) */
  memset(&zero, 0, sizeof(zero));
  const int rc = pa_mtx_read(argv[1], atoi(argv[2]), 0, &A, err, sizeof(err));
  if (rc) {
    printf("error %d %s\nempty %d\n", rc, err, memcmp(&A, &zero, sizeof(A)) == 0);
    return 0;
  }
  const int nnz = A.rowPtr[A.N];
  printf("N %d\nrowPtr %d", A.N, A.N + 1);
  for (int i = 0; i <= A.N; ++i) printf(" %d", A.rowPtr[i]);
  printf("\ncolInd %d", nnz);
  for (int k = 0; k < nnz; ++k) printf(" %d", A.colInd[k]);
  printf("\nval %d", nnz);
  for (int k = 0; k < nnz; ++k) printf(" %.17g", A.val[k]);
  printf("\n");
  pa_mtx_free(&A);
  return memcmp(&A, &zero, sizeof(A)) == 0 ? 0 : 1;
}
