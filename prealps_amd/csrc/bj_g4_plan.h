/*
 * bj_g4_plan.h -- how the band block solve of bj_g4.hip is launched (bj_g4_plan.c): one query of plain ints in, one
 * launch description out.  Everything a launch of k_bj_g4 depends on is decided here and nowhere else: register
 * tiles, column sets, the tiles a record reaches, the occupancy hint, ring depth, wavefronts per workgroup, LDS
 * bytes, grid, whether the Gram by-product rides along and which of the three chains runs.  bj_g4.hip only maps the
 * description onto the template instance that has these numbers compiled in.  Pure host arithmetic on libc: no
 * device call, no environment, no state (tests/c/bj_g4_plan_check.c runs it under the host sanitizers over every
 * dispatch edge).
 */
#ifndef PA_BJ_G4_PLAN_H
#define PA_BJ_G4_PLAN_H

#ifdef __cplusplus
extern "C" {
#endif

/* What the kernels take: rows of a block, bands on one column set (panels of up to 4 columns), bands on two column
 * sets (5 .. 8 columns, and the PAIR launch). */
#define PA_BJ_G4_MAX_ROWS 256
#define PA_BJ_G4_MAX_BAND 112
#define PA_BJ_G4_MAX_BAND8 80
int pa_bj_g4_max_rows(void);
int pa_bj_g4_max_band(void);
int pa_bj_g4_max_band8(void);

/* 1: the one-copy records serve a class with bands up to wmax on a panel of ts columns (`wide` = PREALPS_BJ_G4_WIDE,
 * which the caller reads: 0 keeps 8-column panels with k_bj_mfma) */
static inline int pa_bj_g4_takes_panel(int wmax, int ts, int wide) {
  return ts <= 4 || (ts == 8 && wide && wmax <= PA_BJ_G4_MAX_BAND8);
}

/* ring buffers of the pipelined chain (G4F_RING of bj_g4.hip; one spare buffer more per wavefront) */
#define PA_BJ_G4_PIPE_RING 4

enum { PA_BJ_G4_PLAIN = 0, PA_BJ_G4_PIPE = 1, PA_BJ_G4_PAIR = 2 };

typedef struct {
  int count;              /* blocks of the list */
  int wmax, bmax;         /* widest band, most rows of a block in it */
  int xs, ncol;           /* row stride of the panels in doubles, columns to solve */
  int bits;               /* storage bits of the records: 64 / 32 */
  int gram;               /* 1: a Gram by-product is requested for this launch (pa_k_bj_g4_gram) */
  int cus;                /* compute units of the device (<= 0: unknown, taken as 256) */
  int ring_env;           /* PREALPS_BJ_G4_RING (0: unset) */
  int pair_mode;          /* PREALPS_BJ_PAIR: 0 never, 1 whenever possible, anything else: the default rule */
  int pair_intact;        /* 1: no refresh has split a class of identical blocks since the create */
  int have_tasks;         /* 1: the list has pair tasks, ntasks of them, `paired` blocks with a partner */
  int ntasks, paired;
} pa_bj_g4_query_t;

typedef struct {
  int kind;               /* PA_BJ_G4_PLAIN / _PIPE / _PAIR */
  int nt, nc, dq, occ;    /* template arguments of k_bj_g4: tiles 12 / 14 / 16, column sets, tiles a record reaches,
                             wavefronts per SIMD the registers are bounded for */
  int gp;                 /* 1: the Gram by-product rides along */
  int bits;               /* records read: 64 / 32 */
  int ring;               /* LDS buffers a wavefront's chunks go round (PIPE: PA_BJ_G4_PIPE_RING) */
  int waves;              /* wavefronts per workgroup */
  int per_wave;           /* LDS per wavefront, in doubles */
  int lds;                /* dynamic LDS of a workgroup, in bytes: waves * per_wave * 8 */
  int blocks;             /* workgroups */
  int last[4];            /* what pa_bj_g4_last reports: ring, bits, pipelined, paired */
} pa_bj_g4_launch_t;

/* The launch for q in *L: returns 0, or 1 with the reason (the offending value and its limit) in why[0 .. why_len).
 * The rules are written out in bj_g4_plan.c, next to the code. */
int pa_bj_g4_plan(const pa_bj_g4_query_t* q, pa_bj_g4_launch_t* L, char* why, int why_len);

#ifdef __cplusplus
}
#endif

#endif
