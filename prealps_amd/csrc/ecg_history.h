/*
 * ecg_history.h -- the host side of the solution history (preAlps_SolutionHistory*, preAlps_ECGSolveSystemHistory):
 * pure host arithmetic on libc, like ecg_refine.c and ecg_energy.c.  The history holds the last K <= capacity <= 16
 * solutions of systems on one operator, Xh (N x K, on the device, the glue's business), and their Gram matrix in the
 * energy inner product, G = Xh^T A Xh (K x K, here).  A new solve starts from the element of span(Xh) closest to its
 * solution in the A-norm, x0 = Xh c with G c = Xh^T b (Fischer's projection).
 *
 * Ring.  The columns live in `cap` physical slots.  Until the ring is full a new column takes the next free slot; a
 * full ring overwrites its oldest column.  So the live slots are always 0 .. count - 1, and logical column i (0: the
 * oldest) lies in slot (head + i) % cap, head = 0 until the ring has wrapped.  Raw solutions are kept, not an
 * A-orthonormalised basis: dropping the oldest vector of an orthonormalised history drops the direction every later
 * vector was cleaned of, and the projection loses its dominant component; a raw ring loses one solution.
 *
 * G is stored by physical slot with leading dimension PA_HIST_MAX and is exactly symmetric: every dot product the
 * device formed is stored at (i, j) and at (j, i).  Of the two dots x_a^T (A x_b) and x_b^T (A x_a) that one append
 * of several columns forms for a pair of new columns, the one with the smaller index on the left is kept.  Evicting a
 * column overwrites its row and column.
 *
 * Projection.  With s_i = 1 / sqrt(G_ii) (0 for a column whose G_ii is not positive: an all-zero column) the system
 * is scaled to unit diagonal, Gs = S G S in logical order, and factored by a diagonally pivoted Cholesky that stops
 * when the largest remaining pivot is <= rtol: what is left of the columns not yet taken is, relative to their own
 * A-norm, within sqrt(rtol) of the span of the columns kept (an exact duplicate leaves 0).  Those columns get the
 * coefficient 0, rank = the columns kept.  Then Gs[kept] cs = S g, c = S cs, captured_j = c_j^T g_j = ||x0_j||_A^2.
 * The factor and the triangular solves are the textbook ones, so on the kept set the backward error is that of
 * Cholesky: |Gs cs - gs|_i <= gamma_(3K+1) sum_j (|R^T||R|)_ij |cs_j| <= gamma_(3K+1) (1 + K gamma) ||cs||_1, since the
 * columns of R have norm at most sqrt(1 + ..).  Limits: rtol bounds the conditioning of the kept block only loosely
 * (cond <= about K / rtol); with the default 1e-12 the coefficients can be large and cancel, which the combine's
 * forward bound gamma_K |Xh||c| prices; the caller's guard is that any x0 is a safe start, because the start residual
 * of the solve is formed by a true product.  A G with a NaN or an Inf, or whose largest diagonal entry is not
 * positive, is refused.
 */
#ifndef PA_ECG_HISTORY_H
#define PA_ECG_HISTORY_H

#define PA_HIST_MAX 16
#define PA_HIST_RTOL_DEFAULT 1e-12

enum { PA_HIST_OK = 0, PA_HIST_BAD_ARGS = 1, PA_HIST_BAD_GRAM = 2 };

typedef struct {
  int cap, count, head;                    /* head: the slot of the oldest column */
  double G[PA_HIST_MAX * PA_HIST_MAX];     /* by physical slot, ld PA_HIST_MAX; rows / columns >= count are zero */
} pa_hist_t;

/* 1: capacity lies in 1 .. PA_HIST_MAX */
int pa_hist_capacity_ok(int cap);
/* an empty ring of `cap` slots; PA_HIST_BAD_ARGS and h untouched when the capacity is out of range */
int pa_hist_init(pa_hist_t* h, int cap);
void pa_hist_clear(pa_hist_t* h);
/* the slot of logical column i, 0 <= i < count (0: the oldest); -1 outside */
int pa_hist_slot(const pa_hist_t* h, int i);
/* Append q >= 1 columns (the last cap of them when q > cap).  DO (count x q, ld ldo): the dots of the live columns, by
 * physical slot as they stand BEFORE the call, with the q products w_j = A x_j; DN (q x q, ld ldn): DN[a + j ldn] =
 * x_a^T w_j.  Places the columns in ring order, rewrites the rows and columns of G they take, and leaves in
 * slots[j] the slot column j went to (-1: not kept).  PA_HIST_BAD_GRAM, and h untouched, when a diagonal entry
 * x_j^T w_j is not finite. */
int pa_hist_append(pa_hist_t* h, int q, const double* DO, int ldo, const double* DN, int ldn, int* slots);
/* G again from D = Xh^T (A Xh) (count x count by physical slot, ld ldd), symmetric by the rule above */
int pa_hist_set_gram(pa_hist_t* h, const double* D, int ldd);
/* The pivoted Cholesky and the solve on a system that is already scaled: Gs K x K (ld K, unit or zero diagonal, only
 * read), gs K x q (ld K); cs K x q (ld K) receives the coefficients (0 for a dropped column), piv[0 .. rank) the
 * columns kept in the order they were taken.  Returns the rank. */
int pa_hist_factor_solve(int K, const double* Gs, int q, const double* gs, double rtol, double* cs, int* piv);
/* The projection: g K x q (ld K, K = count, LOGICAL order: row i belongs to the column in pa_hist_slot(h, i)), rtol
 * <= 0: the default; c K x q (ld K, logical order), *rank, captured[q].  An empty history gives rank 0. */
int pa_hist_project(const pa_hist_t* h, int q, const double* g, double rtol, double* c, int* rank, double* captured);

/* Several processes: the buffer one all-reduce of an entry carries, PA_HIST_RED_WORDS = 1 + 16 + 256 + 256 doubles on
 * the device: [failed | 16 sums | a first block of 256 | a second block of 256].  Word 0 is nonzero where a process
 * failed.  A block is column major with the leading dimension of its rows and starts where its region starts:
 *   PA_HIST_RED_PROJECT  a = the q sums b_j^2 (1 x q) at word 1,  b = g = Xl^T b (K x q) at word 17, K >= 0; 273 words
 *   PA_HIST_RED_APPEND   a = DO = Xl^T W (K x q) at word 17, K >= 0,  b = DN = Xn^T W (q x q) at word 273; 529 words
 *   PA_HIST_RED_REFRESH  a = G = Xl^T W (K x K) at word 17, K >= 1,  b empty; q is not looked at; 273 words
 * words: what the all-reduce carries, word 0 included.  Neither the place of entry (i, j) nor the word count of an
 * entry depends on q (nor, for j = 0, on anything but i): a library that sums the processes' shares chunk by chunk of
 * the buffer (the ring of gloo or RCCL) adds them in an order that the place and the count decide, so column j of a
 * projection of q columns has the bits of the same column projected with fewer or more beside it.  The words an
 * entry does not fill are zero (the glue clears the buffer first).  PA_HIST_BAD_ARGS, and l untouched, for an unknown
 * entry or a K or q outside 0 / 1 .. PA_HIST_MAX. */
#define PA_HIST_RED_WORDS (1 + 16 + 256 + 256)
enum { PA_HIST_RED_PROJECT = 0, PA_HIST_RED_APPEND = 1, PA_HIST_RED_REFRESH = 2 };
typedef struct { int off_a, rows_a, cols_a, off_b, rows_b, cols_b, words; } pa_hist_red_t;
int pa_hist_red_layout(int entry, int K, int q, pa_hist_red_t* l);

#endif
