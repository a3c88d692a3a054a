/*
 * pa_alloc.h -- the allocation of large host arrays, shared by the pure host units (spmm_plan.c, mtx_read.c,
 * op_build.c) and operator.c.
 */
#ifndef PA_ALLOC_H
#define PA_ALLOC_H

#include <stddef.h>
#include <stdlib.h>
#include <sys/mman.h>

/* Large host arrays (hundreds of MB, written once): 2 MiB alignment + a transparent-huge-page
 * hint, so that filling them is not dominated by 4 KiB page faults.  Release with free(). */
static inline void* pa_big_alloc(size_t bytes) {
  void* p = NULL;
  if (bytes < ((size_t)8 << 20)) return malloc(bytes ? bytes : 1);
  if (posix_memalign(&p, (size_t)2 << 20, bytes)) return NULL;
  (void)madvise(p, bytes, MADV_HUGEPAGE);
  return p;
}

#endif
