/*
 * bj_band_plan.h -- which kernel family of the band block solve serves a bandwidth class at a panel width, and how it
 * is launched (bj_band_plan.c): one query of plain ints in, one launch description out.  The precedence of the
 * families, the template arguments, the LDS sizing, the grids and the limits are decided here and nowhere else;
 * bj_band.hip only maps the description onto the template instance that has these numbers compiled in, and k_bj_g4
 * has a planner of its own for the rest of its launch (bj_g4_plan.h).  Pure host arithmetic on libc: no device call,
 * no environment, no state (tests/c/bj_band_plan_check.c runs it under the host sanitizers over every dispatch edge).
 */
#ifndef PA_BJ_BAND_PLAN_H
#define PA_BJ_BAND_PLAN_H

#ifdef __cplusplus
extern "C" {
#endif

/* Register sets per lane of the one-wavefront kernels (a class R holds bands up to 64 R - 64), and the widest band
 * of the device's band Cholesky k_bj_factor. */
#define PA_BJ_MAX_R 8
#define PA_BJ_FACTOR_WMAX 96
int pa_bj_max_R(void);
int pa_bj_factor_wmax(void);

/* steps of a block per LDS chunk: the CH of k_bj_apply and k_bj_apply_pairs (k_bj_mfma has it built in) */
#define PA_BJ_BAND_CHUNK 8

enum { PA_BJ_BAND_G4 = 0, PA_BJ_BAND_MFMA = 1, PA_BJ_BAND_APPLY_PAIRS = 2, PA_BJ_BAND_APPLY = 3, PA_BJ_BAND_WIDE = 4 };

typedef struct {
  int ts;                 /* row stride of the panels in doubles: 2 / 4 / 8 / 16 */
  int R, wmax, count;     /* the class: register sets per lane (< 0: wide, -R sets, 1 / 2 / 4), its widest band, its blocks */
  int have_g4, have_pairs;/* 1: the class has one-copy records (bj_g4.hip); 1: paired records exist (k_bj_pairs ran) */
  int g4_wide, mfma;      /* PREALPS_BJ_G4_WIDE and PREALPS_BJ_MFMA, which the caller reads (absent: 1 and 1) */
  int cus;                /* compute units of the device (<= 0: unknown, taken as 256) */
} pa_bj_band_query_t;

typedef struct {
  int family;             /* PA_BJ_BAND_*; G4: nothing below is set, pa_k_bj_g4 plans its own launch */
  int ts, xs, r, ch;      /* template arguments: columns a wavefront solves, row stride of the panels, register sets per
                             lane, steps per chunk (PA_BJ_BAND_CHUNK) */
  int tiles, cap;         /* k_bj_mfma: tiles of 16 rows, 4 / 6 / 8; k_bj_wide: the thread bound of the instance, 768 / 1024 */
  int waves, threads;     /* wavefronts per workgroup, 64 threads each */
  int nbuf, per_wave, lds;/* chunk buffers per wavefront, their doubles, dynamic LDS of a workgroup in bytes: waves * per_wave * 8 */
  int blocks;             /* workgroups */
} pa_bj_band_launch_t;

/* The launch for q in *L: returns 0, or 1 with the reason (the offending value and its limit) in why[0 .. why_len).
 * The rules are written out in bj_band_plan.c, next to the code. */
int pa_bj_band_plan(const pa_bj_band_query_t* q, pa_bj_band_launch_t* L, char* why, int why_len);

#ifdef __cplusplus
}
#endif

#endif
