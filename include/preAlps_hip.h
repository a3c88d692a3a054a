/*
 * preAlps_hip.h -- entry points of libprealps_hip.so that have no counterpart
 * in the reference: device/context management, the process-group hooks, the
 * in-memory operator builder and host<->HBM panel transfers.  Everything a
 * reference driver needs is in preAlps_abi.h; this header is what a new
 * binding (ctypes, cgo, JNI, Fortran ISO_C) adds on top.  Plain C ABI: only
 * pointers, ints, doubles.
 */
#ifndef PREALPS_HIP_H
#define PREALPS_HIP_H

#include "preAlps_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- context ----------------------------------------------------------- */
/* Select the HIP device of this process and create the library's stream.
 * Fails (non-zero) when no gfx950 device is usable: there is no CPU fallback. */
int preAlps_hip_init(int device);
void preAlps_hip_shutdown(void);
/* Run every kernel on the caller's stream (a hipStream_t), e.g. the stream a
 * host framework issues its collectives on.  NULL restores the own stream. */
int preAlps_hip_set_stream(void* hip_stream);
void* preAlps_hip_get_stream(void);
int preAlps_hip_sync(void);
/* 1 (default): errors print "ABORTING from <fn> : [Proc: r] ..." and abort(),
 * like CPLM_Abort (utils/cplm_core/cplm_utils.c:17-58).  0: entry points
 * return non-zero and preAlps_hip_last_error() holds the message. */
void preAlps_hip_set_abort_mode(int abort_on_error);
const char* preAlps_hip_last_error(void);
/* Row stride (in doubles) of a device panel for a given enlarging factor. */
int preAlps_hip_panel_stride(int enlFac);

/* ---- process group ----------------------------------------------------- */
/* One process per GPU.  rank/size describe the processes that share one
 * operator; the library itself never opens a socket: sums and halo rows go
 * through the two hooks, which the host binds to RCCL (torch.distributed
 * backend "nccl", MPI, ...).  Buffers handed to the hooks are device memory
 * (in plan-only mode, where there is no device, the one word on which the ranks
 * agree about a refused start is host memory) and all work queued on preAlps_hip_get_stream() must be ordered before the
 * hook's own communication (the hook is responsible for that ordering). */
typedef int (*preAlps_allreduce_fn)(void* ctx, double* dev_buf, int count);
/* peers[i] sends recv_counts[i] doubles to us and gets send_counts[i] doubles
 * from us; both buffers are packed peer after peer in the order of `peers`. */
typedef int (*preAlps_exchange_fn)(void* ctx, const double* dev_send,
                                   const int* send_counts, double* dev_recv,
                                   const int* recv_counts, const int* peers,
                                   int npeers);
int preAlps_hip_set_world(int rank, int size);
int preAlps_hip_set_comm(preAlps_allreduce_fn allreduce,
                         preAlps_exchange_fn exchange, void* ctx);

/* Built-in hooks: RCCL (ncclAllReduce / grouped ncclSend+ncclRecv over xGMI) on the
 * library stream.  Rank 0 creates the 128-byte id, the launcher broadcasts it, every
 * rank calls preAlps_hip_rccl_init (which also does set_world + set_comm). */
int preAlps_hip_rccl_available(void);   /* 0: librccl.so loads; ranks vote on this before the collective init */
int preAlps_hip_rccl_unique_id(char* id128);
int preAlps_hip_rccl_init(const char* id128, int rank, int size);
/* One shard of a `size`-process run rehearsed in a single process: rank / size as given, the
 * all-reduce hook is the identity and halo rows arrive as zeros (the process then iterates on its own
 * diagonal block of the partitioned matrix with the launches of a real rank).  For measurements. */
int preAlps_hip_loopback(int rank, int size);
/* Collective: checks the installed hooks with one all-reduce and one ring exchange. */
int preAlps_hip_comm_selftest(void);

/* ---- operator from memory ---------------------------------------------- */
/* Same pipeline as preAlps_OperatorBuild (utils/operator.c:38-134) with the
 * matrix taken from memory instead of a MatrixMarket file and an explicit
 * partition vector instead of METIS:  [scale: A <- D A D]  ->  rows grouped
 * part by part (original order inside a part)  ->  symmetric permutation  ->
 * row panel of this process (parts [rank*nparts/size, (rank+1)*nparts/size)).
 * part == NULL selects part[r] = floor(r*nparts/N).  Every process passes the
 * whole matrix (global CSR, 0-based, full symmetric pattern). */
int preAlps_OperatorBuildFromCSR(int N, const int* rowPtr, const int* colInd,
                                 const double* val, int nparts, const int* part,
                                 int scale);
/* New values for the operator built by preAlps_OperatorBuildFromCSR, same sparsity pattern, partition and scale
 * flag: val holds the values of the whole matrix in the order of that build's val (global CSR, rowPtr[N] entries),
 * and every process passes all of it.  The result is the operator that preAlps_OperatorFree followed by
 * preAlps_OperatorBuildFromCSR(the same N, rowPtr, colInd, nparts, part, scale; val) would give, bit for bit -- the
 * host panel seen through preAlps_OperatorGetA and every later preAlps_BlockOperator product -- without the
 * diagonal check, the ordering, the row sort, the halo and peer lists, the cut of the SpMM plan and its upload.  A
 * time step or a Newton step with a changed coefficient is the caller this is for.  No communication: any world size.
 *   Scaling: an operator built with scale gets its scaling vector from the new values, d_i = sqrt(1 / max_j |a_ij|),
 * and the panel value d_i * a_ij * d_j in that order of multiplication, as at the build; a row whose new values are
 * all zero gives the build's error ("Impossible to scale the matrix, rcmin=0").
 *   Addresses stay: the arrays handed out by preAlps_OperatorGetA keep their addresses (A.val shows the new values:
 * a copy of the struct stays valid), and so do the device arrays of the SpMM plan ("spmm_val_address",
 * "spmm_slot_address" of preAlps_hip_get_stat), so a HIP graph captured by the driver loops stays valid.
 *   Plans: with no SpMM plan yet only the host panel changes and the next product cuts its plan from the new values;
 * an existing plan gets its values rewritten on the device by one kernel, through a map (4 bytes per stored value,
 * kept on the device, cut at the first update of a plan) from stored value to panel entry.  A later change of the
 * panel stride cuts the plan from the new host panel as always and drops the map.  Plan-only mode: host part only.
 *   Ordering: the device work is queued on the library stream, behind earlier products; the entry returns when val
 * and the host panel are free again and the kernel has finished.  Call it between solves: a solver in the middle of
 * an iteration would go on with panels of the old matrix.
 *   The preconditioner is not touched: the block-Jacobi factor of the old values stays in place -- it is still
 * symmetric positive definite, a lagged preconditioner for the new matrix -- and preAlps_BlockJacobiFree +
 * preAlps_BlockJacobiCreate on the updated A give the fresh one, preAlps_BlockJacobiUpdateValues (below) the same
 * factor in place.  "op_values_epoch" (0 after a build, + 1 per
 * successful update) against "bj_values_epoch" (that count at the last create or refactorisation) tells a lagged
 * factor; "op_value_map_builds" and "op_value_map_bytes" count the maps cut for this operator and the device bytes
 * of the current one; "op_update_host_s" / "op_update_copy_s" / "op_update_kernel_s" are the last update's host
 * seconds (scaling vector and panel), the host seconds of the copy of the panel values to the device and the device
 * seconds of the kernel, "op_update_map_s" the host seconds the last map took.
 *   Refused, the operator left as it was (the message names this entry point): no operator built; an operator that
 * preAlps_OperatorBuild read from a file (the order of its values is not the caller's); val == NULL; the zero row
 * above; no memory for the scaling vector, the map or the device copy of the panel values. */
int preAlps_OperatorUpdateValues(const double* val);
/* The block-Jacobi preconditioner follows an update of the values: a numeric refactorisation in place.  No argument:
 * the values are the library's own host panel, as preAlps_OperatorGetA shows it after preAlps_OperatorUpdateValues.
 *   Band blocks (every block without the sparse factor): the result is the preconditioner that
 * preAlps_BlockJacobiFree + preAlps_BlockJacobiCreate on the current panel would give, bit for bit -- the plain
 * records of both sweeps, 1 / L(j,j), the one-copy records (fp64 or fp32, in the storage of the create that is being
 * refreshed) and the paired records -- without what depends on the pattern alone: the adjacency graphs, the orders,
 * the bandwidths, the dispatch classes, the record offsets, the index arrays, the class lists, the host assembly of
 * the bands and their upload.  The decisions of the create are kept with the preconditioner; no switch of the
 * environment is read again.  The panel values go up in one copy, the bands are assembled on the device through
 * the band map (below), and the band Cholesky and the layout kernels of the create run on the create's lists.
 *   Addresses stay: no device array of the band factor is freed or allocated again ("bj_records_address",
 * "bj_g4_address" of preAlps_hip_get_stat show two of them), so a HIP graph that captured an apply stays valid.
 * The assembled bands and the copy of the panel values are temporary device memory inside the call, as in the create.
 *   The band map: one entry of 8 bytes for every panel entry inside a band block's diagonal block, on or below the
 * diagonal in factor order -- 4 bytes for its index in the panel's val, 4 for its place inside its block's band --
 * and a list of chunks (block, first entry).  It is cut at the first update after a create, so a caller who never
 * updates pays nothing, and stays on the device until the preconditioner is freed.
 *   Blocks with the sparse (nested-dissection) factor are NOT refreshed in place: the library does not keep their
 * symbolic structure, so they are created again from the new panel with the arguments and the storage of the create,
 * and THEIR device arrays move ("bj_update_nd_rebuilt" = the number of blocks refreshed this way).  Band blocks of
 * the same preconditioner still take the path above.
 *   Stats: "bj_values_epoch" becomes "op_values_epoch"; "bj_updates" counts the successful updates since the create;
 * "bj_band_map_builds", "bj_band_map_entries", "bj_band_map_bytes"; "bj_update_map_s" / "bj_update_copy_s" are the
 * host seconds of the last map cut (with its upload) and of the last copy of the panel values, "bj_update_kernel_s"
 * the device seconds between two events around assembly, factorisation and second layouts, "bj_update_total_s" the
 * host wall seconds of the whole call.
 *   Ordering: the work is queued on the library stream behind earlier applies, and the entry returns when the new
 * factor is in place.  No communication: any world size.  Call it between solves.
 *   Refused, the factor left exactly as it was (the message names this entry point; every refusal and every allocation
 * of the band path comes before the first write into the factor): no preconditioner created; no operator built, or
 * one freed or built again since the create; a create whose A was not the operator's own panel; a preconditioner
 * created with PREALPS_BJ_FACTOR=host, whose records come from the host Cholesky (free and create instead); a band of
 * 2^32 entries or more; no memory for the map, the values or the bands.
 *   New values that are not SPD: the kernels have overwritten the records by the time a pivot fails, so the old
 * factor cannot be kept.  The entry reports "diagonal block is not SPD (global row r)" as the create does and frees
 * the preconditioner, as a failed create does (so does any device error after the first write, and a failure of the
 * sparse blocks' create); a later preAlps_BlockJacobiCreate works. */
int preAlps_BlockJacobiUpdateValues(void);
/* ---- two-level block Jacobi: an additive coarse correction from given vectors -----------------------------------
 * Block Jacobi has no coarse space, so its iteration count grows with the number of blocks.  With k vectors V near the
 * kernel of A (the translations or the rigid-body modes of an elasticity problem, the constant of a diffusion problem)
 * the preconditioner becomes M^-1 = B^-1 + Z E^-1 Z^T: B^-1 is the block-Jacobi apply as it is, band and sparse
 * factors alike; Z holds the vectors cut aggregate by aggregate -- an aggregate is a set of parts, row i of a part in
 * aggregate g has its k values in the columns g*k .. g*k + k - 1 -- and E = Z^T A' Z with A' = P D A D P^T the
 * operator's own matrix, nc = naggr * k unknowns.  M^-1 is symmetric positive definite whenever E is; the ECG
 * iteration needs nothing else.  Opt-in: without this call nothing changes, bit for bit.
 *   V: N x k column major, ldv >= N, 1 <= k <= 8, in the order and units of the matrix the operator was built from,
 * as b of preAlps_ECGSolveSystem; internally Vp = (D^-1 V)[perm] (a vector near the kernel of A is near the kernel
 * of D A D after division by d).  part_aggregate: nparts ints in [0, naggr), every aggregate non-empty; NULL selects
 * one aggregate per part when nparts * k fits the cap, otherwise floor(cap / k) aggregates from
 * preAlps_hip_partition_kway on the quotient graph of the parts (an edge where some a_ij joins two parts).
 *   Set-up (host, fp64, the same bits for any number of threads): E is assembled by aggregates in row order, factored
 * by Cholesky, and Einv = L^-T L^-1 is formed explicitly and made symmetric in bits; a pivot <= nc * eps * max diag E
 * refuses the vectors and names the aggregate and the vector.  The cap on nc is "bj_coarse_max_dofs" (1536: 18.9 MB
 * of Einv on the device, about nc^3 host flops).
 *   Apply: preAlps_BlockJacobiApply adds Z Einv Z^T in to out after the block solve, over the live columns, with three
 * stages of coarse.hip: a pass over `in` that leaves one k x columns block per chunk of at most 1024 rows, the sum of
 * each aggregate's blocks in list order and one streaming pass over Einv, and a read-modify-write pass over `out`.
 * No atomics: two applies of one input agree in bits.  While a coarse space is attached the block solve does not
 * leave the Gram block of the iteration behind ("bj_gram_applies" stays), and the solver takes the path of
 * PREALPS_BJ_GRAM=0, also a solver initialised before the call.
 *   Values: preAlps_BlockJacobiUpdateValues forms zv, E and Einv again from the kept V (8 k N bytes on the host) and
 * aggregates and the new values and scaling vector, into the same device arrays ("bj_coarse_einv_address" stays); a
 * singular E there drops the coarse space and reports, the refreshed block factor stays.  After
 * preAlps_OperatorUpdateValues alone the coarse space is lagged with the factor, still SPD.
 * preAlps_BlockJacobiFree releases it; setting one again replaces it.
 *   Solvers: set, replace or clear between solves.  Both entries drain the library stream first.  A solver that replays
 * HIP graphs (preAlps_hip_graphs) notices the change at its next iteration and captures its segments anew, as it does
 * after preAlps_BlockJacobiFree + Create; a solver in the middle of an iteration goes on with the new apply.
 *   Stats: "bj_coarse_dofs", "bj_coarse_vectors", "bj_coarse_aggregates", "bj_coarse_chunks", "bj_coarse_bytes"
 * (device), "bj_coarse_setup_s" (host seconds of the last build with its upload), "bj_coarse_builds" (the set and
 * every refresh since), "bj_coarse_applies", "bj_coarse_einv_address": 0 without a coarse space; and
 * "bj_coarse_max_dofs".
 *   Several processes (preAlps_hip_set_world / the MPI binding): the call is collective and gives the Z and E one
 * process would form from the same matrix, partition, vectors and aggregates.  Every rank passes the same global V (all
 * N rows, as b of preAlps_ECGSolveSystem) and the same part_aggregate -- nparts entries for the parts of ALL ranks, an
 * aggregate may span ranks -- or NULL: one aggregate per part when the global nparts * k fits the cap, otherwise every
 * rank cuts the quotient graph of its own parts (edges to other ranks' parts dropped) into max(1, floor(floor(cap / k)
 * * np_rank / nparts)) aggregates, numbered rank after rank, so that no default aggregate spans ranks.  Every rank forms
 * its share E_r from its own rows, the shares are summed by the all-reduce hook, and every rank factors the same bits:
 * a singular E is refused on all ranks alike; what one rank alone meets (a non-finite entry in its copy of V, no
 * memory, a failed upload) is agreed on before any rank returns, and the ranks not at fault report that another process
 * refused.  The device keeps the rows of Einv that the rank's own aggregates need ("bj_coarse_bytes" is the rank's
 * own), and an apply costs exactly one all-reduce more (of the nc x stride coarse vector, on the library stream).
 * preAlps_BlockJacobiUpdateValues refreshes collectively; preAlps_BlockJacobiClearCoarseSpace must be called on every
 * rank.  Nothing about speed on two or more devices has been measured.
 *   Refused, the preconditioner left as it was (a coarse space set earlier included) -- on several processes on every
 * rank: no operator or no preconditioner; a preAlps_hip_loopback shard (it lacks the other ranks' rows of E); plan-only
 * mode; k out of range; ldv < N; a non-finite entry of V; naggr * k above the cap; an empty aggregate or one out of
 * range; a singular E. */
int preAlps_BlockJacobiSetCoarseSpace(int k, const double* V, int ldv, const int* part_aggregate, int naggr);
int preAlps_BlockJacobiClearCoarseSpace(void);
/* The aggregates of the attached coarse space: part_aggregate[p] for every part (nparts ints, the caller's array; on
 * several processes the parts of all of them) -- what the caller gave, or the default the library chose -- and *naggr
 * (may be NULL).  Refused without a coarse space. */
int preAlps_BlockJacobiGetCoarseAggregates(int* part_aggregate, int* naggr);
/* k-way partition of the adjacency graph of a square matrix with a structurally symmetric
 * pattern (0-based CSR, diagonal stored) into nparts compact, balanced parts:
 * part[i] in [0, nparts) for every row i.  This is what the library calls in place of the
 * reference's METIS_PartGraphKway (utils/cplm_core/cplm_matcsr_core.c:394-457); consecutive
 * part ids are neighbouring regions, so a process that owns a range of ids owns a compact
 * piece of the domain.  Host code: needs no GPU. */
int preAlps_hip_partition_kway(int N, const int* rowPtr, const int* colInd, int nparts, int* part);
/* Host-side self check of the sparse factorisation that large diagonal blocks get (nested
 * dissection + multifrontal Cholesky, nd.c), on one SPD matrix taken as a single block; no GPU
 * needed.  stats[0..7] = supernodes, doubles of one panel copy, rows of the largest front, tree
 * height, ||L L^T x - A x|| / ||A x||, largest relative mismatch between the two panel copies,
 * largest deviation of the selective-inversion panels [T ; -G] from T (I + Lhat_11) = I and
 * G (I + Lhat_11) = Lhat_21, pivot columns of the widest supernode. */
int preAlps_hip_nd_selfcheck(int n, const int* rowPtr, const int* colInd, const double* val, int leaf_rows,
                             double* stats);
/* Cut the SpMM plan (slices, LDS staging lists) for this enlarging factor now rather than
 * inside the first preAlps_BlockOperator call; optional. */
int preAlps_hip_prepare_operator(int enlFac);
/* Plan-only mode: build the sharding and halo lists on the host without a GPU
 * (used by the multi-process CPU tests); preAlps_BlockOperator is refused. */
void preAlps_hip_plan_only(int on);
/* The halo plan of this process (library-owned arrays): peers[i] gets
 * send_rows[i] of our rows (local row ids in send_idx, peer after peer) and
 * owns recv_rows[i] of our halo slots (their global rows in halo_cols). */
int preAlps_OperatorGetHaloPlan(int* npeers, int** peers, int** send_rows, int** recv_rows,
                                int** send_idx, int* nsend, int** halo_cols, int* nhalo);
/* The inverse of send_idx, as the solver's update kernel uses it to pack the send buffer itself (several processes,
 * DESIGN section 5): local row r goes into the send-buffer slots slot_out[off_out[r] .. off_out[r + 1]).
 * off_out: m + 1 ints, slot_out: nsend ints (caller's arrays).  Works in plan-only mode. */
int preAlps_hip_pack_map(int* off_out, int* slot_out);
/* Where preAlps_ECGInitializeMulti / Guess put a local row at s columns per system: pcol[i] = p % s for a row of part
 * p, p the global index of the part, so the shards of several processes hold slices of the one-process array.
 * pcol: m ints (caller's array).  Works in plan-only mode. */
int preAlps_hip_system_columns(int s, int* pcol);
/* perm[new] = old, of the whole problem (library-owned, N ints). */
int preAlps_OperatorGetPermPtr(int** perm, int* n);
int preAlps_hip_nparts(void);

/* ---- helpers for drivers and tests ------------------------------------- */
/* The rhs of examples/test_ecg_prealps_op.c:172-184 for the local rows, as a
 * run of the reference with np = nparts ranks would build it. */
int preAlps_hip_reference_rhs(double* rhs_local);
/* The driver loop of examples/test_ecg_prealps_op.c:203-223 (fused variant:
 * examples/test_ecg_bench_fused.c:243-259). res_hist may be NULL. */
int preAlps_ECGSolve(preAlps_ECG_t* ecg, double* rhs, double* sol,
                     double* res_hist, int* bs_hist, int max_hist, int* n_hist);
/* ---- several right-hand sides on one operator ---------------------------------------------------------------
 * The ECG iteration is block CG on an m x enlFac panel, so started from R0 = [b_1 | ... | b_k] it solves k systems
 * in one pass over the matrix and the block factors per iteration.  nrhs = k >= 1; ecg->enlFac must be a multiple of
 * k and s = enlFac / k is the enlarging factor of each system: system j owns the columns j*s .. j*s + s - 1 of X, R,
 * P ..., and a row of part p puts b_j into column j*s + (p % s) (k = 1: the split of preAlps_ECGInitialize).  rhs:
 * the local rows, column major, ldrhs >= m.  Every system converges in the block Krylov space of all of them.
 *   Iteration: that of one system at the same ortho_alg, bs_red and enlFac, launch for launch, plus one small launch
 * per iteration that sums the residual columns of each system.  A solver started here runs under the caller's own
 * loop of preAlps_ECGIterate / preAlps_BlockOperator / preAlps_BlockJacobiApply / preAlps_ECGStoppingCriterion.
 *   Stopping: g_j = Frobenius norm of the columns of R that belong to system j, normb_j = ||b_j||_2; the iteration
 * goes on while g_j > tol * normb_j for some j (and iter < maxIter, bs > 0; a NaN stops it).  Systems that have
 * converged keep iterating with the rest (no deflation).  ecg->res stays the Frobenius norm of all of R,
 * ecg->normb = ||B||_F.  With k = 1 this is the test of preAlps_ECGStoppingCriterion as it always was.
 *   Finish: x_j = the sum of the columns of system j of X, written to sol[i + j*ldsol], ldsol >= m.
 *   Accuracy: the true residual of system j is the sum of its s columns of R, so in exact arithmetic
 * ||b_j - A x_j|| <= sqrt(s) * g_j (Cauchy-Schwarz); s = 1: they are equal.
 *   Refused (non-zero / abort, the message names the entry point): nrhs < 1 or enlFac % nrhs != 0; s larger than
 * the number of parts; ldrhs or ldsol < m; a right-hand side of norm zero (its columns of R0 would be empty);
 * ORTHODIR_FUSED (it decides inside preAlps_ECGIterate on one sum); preAlps_ECGFinalize and preAlps_ECGAdvance on a
 * solver that holds more than one system.  HIP graphs (preAlps_hip_graphs, PREALPS_ECG_GRAPH) and PREALPS_ECG_POLL
 * are off for such a solver.
 *   Several processes (and a preAlps_hip_loopback shard, which rehearses one of them with empty collectives): as for
 * preAlps_ECGSolve every rank passes its own m rows; rhs, x0 and sol are local.  sys_normb, the per-system histories,
 * preAlps_ECGSystemResiduals, ecg->res and ecg->normb hold global values, equal on all ranks: the start sums b_j^2
 * (and, with a guess, the columns of R0) over the ranks in one all-reduce, and in the iteration the k local sums ride
 * behind the residual norm in the collective that carries it anyway (2 + k words where one system reduces its norm,
 * the block beta and 2 + k words with the lazy stopping test), so an iteration gains no collective.  ORTHODIR and
 * ORTHOMIN with NO_BS_RED.  Refused there as well: bs_red = ADAPT_BS with more than one system or a guess; an
 * operator that was built before preAlps_hip_set_world / preAlps_hip_loopback changed the process group (the message
 * is the one that asked for a single process).  A refusal that depends on one rank's arguments or resources (ldrhs,
 * ldx0, locPbSize, an allocation) is agreed on by all ranks before any of them returns -- the rank at fault reports its
 * reason, the others "another process of the group refused" -- and a norm that is zero or not finite is judged on
 * the global sum: no rank is left waiting in a collective.
 *   Linearly dependent right-hand sides (a repeated load case, say) make P^T A P singular: keeping them apart is the
 * caller's business; bs_red = ADAPT_BS drops the directions that have become dependent. */
int preAlps_ECGInitializeMulti(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, int* rci_request);
/* after a stopping test: g_j and normb_j of every system (either pointer may be NULL) */
int preAlps_ECGSystemResiduals(preAlps_ECG_t* ecg, double* sys_res, double* sys_normb);
int preAlps_ECGFinalizeMulti(preAlps_ECG_t* ecg, double* sol, int ldsol);
/* the library's own loop: res_hist / bs_hist as preAlps_ECGSolve; sys_hist (may be NULL) receives
 * g_j of iteration i at sys_hist[i + j * max_hist]; sys_normb (may be NULL): nrhs values */
int preAlps_ECGSolveMulti(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs, double* sol, int ldsol,
                          double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                          int max_hist, int* n_hist);
/* ---- a start from an initial guess, for one and several systems -------------------------------------------------
 * preAlps_ECGInitializeMulti / preAlps_ECGSolveMulti with a starting value x0 for every system: the local rows,
 * column major, nrhs columns, ldx0 >= m.  x0 == NULL: those two entries themselves, the same code path and the same
 * bits (sys_res0, if given, then receives ||b_j||).  Every existing entry keeps its behaviour and its bits.
 *   Start: the iteration needs nothing new.  The solution of system j is the sum of its s columns of X and its
 * residual the sum of its columns of R, so X0 is written by the placement rule above -- a row of part p puts x0_j into
 * column j*s + (p % s), zero elsewhere, and the sum of the columns is x0_j bit for bit -- and R0 is the same split of
 * r0_j = b_j - (the sum of system j's columns of A X0, added in ascending column order); every later update keeps
 * sum_c R(:, c) = b_j - A sum_c X(:, c).  A X0 is one product of the library's own SpMM at the solver's width (the
 * path of preAlps_BlockOperator, no new plan, no Gram block asked of it); the panel it is written to is zeroed again.
 *   Norms and stopping: sys_normb[j] = ||b_j|| and ecg->normb = ||B||_F as without a guess -- the test stays relative
 * to the right-hand side, not to r0.  g0_j = the Frobenius norm of system j's columns of R0, formed on the device.
 * After the initialise preAlps_ECGSystemResiduals returns g0_j and ecg->res is ||R0||_F.  preAlps_ECGInitializeGuess
 * followed by preAlps_ECGSystemResiduals (and preAlps_ECGFinalizeMulti to release the solver) is therefore also the
 * library's answer to "what is ||b - A x|| for this x", in fp64 from the iterate: a residual refresh after a long
 * run or after a solve with the opt-in fp32 factors (s = 1: exactly that norm; s > 1: the norm of its split, which
 * bounds it by sqrt(s)).
 *   Already converged: if g0_j <= tol * ||b_j|| for every j, preAlps_ECGSolveGuess does no iteration: *n_hist = 0,
 * ecg->iter = 0, sol receives x0 bit for bit, and nothing of the iteration is queued, neither the block solve nor
 * the product.
 *   Refused (the message names the entry point): everything preAlps_ECGInitializeMulti refuses (nrhs, divisibility,
 * s against the number of parts, ldrhs, a right-hand side of norm zero, ORTHODIR_FUSED; on several processes
 * ADAPT_BS and a process group changed since the build); ldx0 < m; a start residual that is not finite (NaN or Inf in x0), which reports the
 * system; and a system whose r0_j is exactly zero beside one whose is not ("system %d starts with a zero residual
 * ..."): its columns of the block would be empty and P^T A P singular, as with a zero right-hand side.  A small but
 * nonzero start residual is no error: a system that starts at 1e-8 ||b_j|| iterates beside systems that start at
 * ||b_j|| (the Cholesky factorisation is invariant to the scaling of the columns) and stays converged.  With
 * bs_red = ADAPT_BS it is not known whether the reduction's threshold drops the columns of such a system; as with
 * linearly dependent right-hand sides above, that combination is the caller's business.
 *   Afterwards: preAlps_ECGAdvance is refused on a solver started from a guess, because it restarts from rhs alone
 * and would drop x0.  preAlps_ECGFinalize (one system) and preAlps_ECGFinalizeMulti work unchanged;
 * _preAlps_ECGReset makes the solver a cold one again; the caller's own loop of preAlps_ECGIterate /
 * preAlps_BlockOperator / preAlps_BlockJacobiApply / preAlps_ECGStoppingCriterion works as after
 * preAlps_ECGInitializeMulti.  HIP graphs and PREALPS_ECG_POLL are off for such a solver, as for several systems;
 * the order of the iteration (solve first, lazy normalisation, lazy stopping test) is decided by the solver's
 * description as always: the start is outside the loop. */
int preAlps_ECGInitializeGuess(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs,
                               const double* x0, int ldx0, int* rci_request);
/* preAlps_ECGSolveMulti around that start; sys_res0 (may be NULL): the nrhs start residuals g0_j */
int preAlps_ECGSolveGuess(preAlps_ECG_t* ecg, int nrhs, const double* rhs, int ldrhs,
                          const double* x0, int ldx0, double* sol, int ldsol,
                          double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                          double* sys_res0, int max_hist, int* n_hist);
/* ---- the caller's own system: original order, scale and residual norm -------------------------------------------
 * Every entry above works in the operator's internal space: it takes the right-hand side and returns the solution of
 * A' = P D A D P^T, where P groups the rows part by part (preAlps_OperatorGetPermPtr: perm[new] = old) and D = diag(d),
 * d_i = sqrt(1 / max_j |a_ij|), is the scaling of preAlps_OperatorBuild and of preAlps_OperatorBuildFromCSR with
 * scale != 0.  The entries below solve A x = b as the caller stated it, on one process (N = m) or on several.
 *   Several processes (collective calls; a preAlps_hip_loopback shard counts as one of several): b, x0 and x stay what
 * they are for one process -- columns indexed by the caller's GLOBAL row, leading dimension >= N, on the host or on the
 * device -- and every rank passes arrays of that shape.  A rank reads only the rows it owns, perm[row_off .. row_off + m)
 * (preAlps_OperatorGetOwnedRows), and writes only those rows of x: every other row of the caller's x keeps its bits, so
 * a sum over the ranks of arrays that started at zero is the whole solution.  sys_res, sys_normb, sys_hist, res_hist,
 * ecg->res, ecg->normb and the iteration count are global, the same words on every rank.  Host arrays go up whole (N
 * doubles per column; the gather picks the owned rows), so no rank makes a host pass over the permutation.  With
 * PREALPS_SYS_STOP_ORIGINAL the per-system sums travel in the collective that carries the residual norm anyway: an
 * iteration costs no all-reduce more than one of preAlps_ECGSolve on the same ranks; the start costs one more than that
 * of preAlps_ECGSolveGuess, and without the flag the finish has one for sys_res.  What one rank alone can find wrong --
 * a leading dimension, a NaN in its rows, a failed allocation -- is agreed on before any rank returns: that rank
 * returns its reason, the others "another process of the group ...".
 *   preAlps_OperatorGetOwnedRows: *rows = perm + row_off (library-owned, the caller's rows this process owns, in the
 * operator's local order) and *m = their count; one process: the whole permutation.  Works in plan-only mode.
 *   preAlps_OperatorGetScalingPtr: the vector d, N doubles, entry i for row i of the matrix the operator was built
 * from (the caller's order).  The array is library-owned; preAlps_OperatorUpdateValues writes the new vector into the
 * same allocation (after its last refusal: a refused update leaves the old one), preAlps_OperatorFree releases it.
 * *d = NULL with *n = N: the operator is unscaled.  Works in plan-only mode and for any number of processes (every
 * process holds the whole vector).
 *   preAlps_ECGSolveSystem is preAlps_ECGSolveGuess around a gather and a scatter.  b, x0 (may be NULL: no guess) and
 * x hold N rows in the order and units of that matrix -- the CSR arrays of preAlps_OperatorBuildFromCSR, the rows of
 * the file -- column major, nrhs columns, ldb, ldx0, ldx >= N.  One launch forms b' = (D b)[perm] and x0' =
 * (D^-1 x0)[perm] (a true division) in the staging arrays of the start and leaves ||b_j||^2 in the caller's units; one
 * launch at the end writes x[perm[i]] = d[perm[i]] * (the solution of the scaled system); b and x0 are only read.
 * The row map on the device (12 bytes per row: perm and d[perm]) is cut at the first call and again after
 * preAlps_OperatorUpdateValues (stats "op_system_map_builds", "op_system_map_bytes").
 *   flags: PREALPS_SYS_DEVICE: b, x0 and x are device pointers.  They are read and written on the library stream and
 * the entry returns after that stream has drained, as the solve loops do; the caller orders their own stream before
 * the call.  Without it they are host arrays.
 *   PREALPS_SYS_STOP_ORIGINAL: the iteration goes on while ||b_j - A x_j|| > tol * ||b_j|| for some j, both norms in
 * the caller's units (and iter < maxIter, bs > 0; a NaN stops it), for one system as for several.  The left side is
 * the recurrence residual: the sum of system j's columns of R is that system's whole residual in the scaled space
 * (every update keeps sum_c R(:, c) = b'_j - A' sum_c X(:, c)), and divided row by row by d[perm] it is b_j - A x_j.
 * Its norm is the norm itself, not the sqrt(s) bound of the split.  It costs one more pass over the R panel and one
 * small launch per iteration.  Without the flag the test is the library's: ||D (b_j - A x_j)|| split over its columns
 * against ||D b_j||, the test of preAlps_ECGSolveGuess; with a graded coefficient the two differ by orders of
 * magnitude.  ecg->res and ecg->normb stay the scaled Frobenius norms under both, and so does res_hist.
 *   sys_hist (may be NULL; entry i of system j at sys_hist[i + j * max_hist]) and sys_normb (may be NULL) are in the
 * metric of the stopping test.  sys_res (may be NULL) always receives the nrhs recurrence residual norms in the
 * caller's units at the end, from one more launch after the loop; with PREALPS_SYS_STOP_ORIGINAL that is the last row
 * of sys_hist bit for bit.
 *   Without PREALPS_SYS_STOP_ORIGINAL the iterate, the histories and the iteration count are those of
 * preAlps_ECGSolveGuess (x0 == NULL: preAlps_ECGSolveMulti) on (D b)[perm] and (D^-1 x0)[perm], bit for bit, and
 * x[perm[i]] is d[perm[i]] times its solution.  The start always goes through the device kernels of several systems
 * (pa_k_multi_start, or the three of a guess), also for one system without a guess; for that case the scaled
 * right-hand side comes back to the host once (m doubles) so that ecg->normb is summed as _preAlps_ECGReset sums it.
 *   A guess under which every system already meets its threshold, in whichever metric is selected, comes back as x,
 * bit for bit, after no iteration (*n_hist = 0).
 *   Refused (the message names the entry point): everything preAlps_ECGInitializeGuess refuses -- nrhs < 1 or
 * enlFac % nrhs != 0, s against the number of parts, ORTHODIR_FUSED, an operator built for another process group than
 * the one that calls, ADAPT_BS on several processes, a right-hand side of norm zero, a start residual that is not finite, a system that starts at exactly zero
 * beside ones that do not -- and ldb, ldx0 or ldx < N, b or x == NULL, a right-hand side that is not finite, unknown
 * flags.  After a refusal the operator and the preconditioner are usable as before.  HIP graphs and PREALPS_ECG_POLL
 * are off for such a solver, as for several systems.  The solver object is released before the entry returns.
 *   preAlps_OperatorSystemResiduals: res[j] = ||b_j - A x_j|| and normb[j] = ||b_j|| (either may be NULL) in the
 * caller's units, fresh -- formed from b and x, not from a recurrence: one start from the guess x at s = 1 on a
 * temporary solver of width nrhs (the gather, the library's own product, R0), the norm kernel on R0, and a free.
 * nrhs <= 16 (what the per-system arrays of a solver hold); flags: PREALPS_SYS_DEVICE or 0.  No preconditioner is
 * needed.  It refuses what the start refuses (a zero or non-finite right-hand side, a non-finite x, an operator built
 * for another process group); a residual of exactly zero is an answer here, not a refusal.  Several processes:
 * collective, x is read at the owned rows, its halo comes through the library's exchange, and the sums are reduced. */
#define PREALPS_SYS_DEVICE        1   /* b, x0, x are device pointers */
#define PREALPS_SYS_STOP_ORIGINAL 2   /* stop on ||b_j - A x_j|| <= tol ||b_j|| in the caller's units */
int preAlps_OperatorGetScalingPtr(double** d, int* n);
int preAlps_OperatorGetOwnedRows(int** rows, int* m);
int preAlps_ECGSolveSystem(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb,
                           const double* x0, int ldx0, double* x, int ldx, int flags,
                           double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                           double* sys_res, int max_hist, int* n_hist);
int preAlps_OperatorSystemResiduals(int nrhs, const double* b, int ldb, const double* x, int ldx,
                                    int flags, double* res, double* normb);
/* preAlps_ECGSolveSystem in passes, each measured against the matrix as the caller gave it.  Pass 0 is
 * preAlps_ECGSolveSystem with these arguments as it is.  Every later pass is the same solve started from the x of the
 * pass before it; the product A x of that start always runs on the fp64 values of the matrix, whatever storage the
 * iteration reads (preAlps_hip_set_operator_precision), so the start residual of pass p is a fresh b - A x of the
 * given system.  A start under which every system meets its threshold comes back after no iteration, as a converged
 * guess does from preAlps_ECGSolveSystem, and ends the chain.  With fp32 storage this is iterative refinement with
 * an inner solver on the rounded matrix; with fp64 storage it is a restart with the residual replaced.
 *   max_passes: 1 .. 16 passes may iterate.  ecg->maxIter bounds the iterations of all passes together: a pass gets
 * what is left; ecg->iter holds their sum at the end.  pass_iters: max_passes ints, the iterations of every pass.
 * pass_res: (max_passes + 1) x nrhs doubles, row p (pass_res[p * nrhs + j]) = the start residuals of pass p in the
 * metric of the stopping test -- row 0 those of x0 (||b_j|| without a guess), row p >= 1 the fresh residuals of what
 * pass p - 1 left.  *n_passes: the passes that iterated; row *n_passes holds the residuals that ended the chain.
 * res_hist, bs_hist and sys_hist hold the histories of the passes one behind the other, *n_hist entries in all;
 * sys_normb is that of pass 0.  sys_res: ||b_j - A x_j|| of the x handed back, in the caller's units -- where the
 * chain ended at a start, fresh from the fp64 product, also when x is the iterate before the last pass (below).
 * ecg->res and ecg->normb are the scaled Frobenius norms of the last start or iteration that ran, not those of x.
 *   *status, the first that applies before a pass p >= 1 iterates, with q = max_j res_j / (tol ||b_j||):
 * PREALPS_REFINE_CONVERGED (q <= 1), PREALPS_REFINE_OUT_OF_ITERATIONS (the passes so far have used ecg->maxIter),
 * PREALPS_REFINE_STAGNATED (p >= 2 and pass p - 1 did not halve q), PREALPS_REFINE_OUT_OF_PASSES (p = max_passes).
 * All four return 0.  With the three that are not CONVERGED x is the better of the iterates before and behind the
 * last pass -- a pass that the budget cut short may not have recovered from its restart yet -- so its residuals are
 * row *n_passes or row *n_passes - 1 of pass_res, whichever has the smaller ratio.  (ecg_refine.h states the rule.)
 *   Refused: what preAlps_ECGSolveSystem refuses, max_passes outside 1 .. 16, nrhs > 16, a NULL among n_passes,
 * pass_iters, pass_res and status.  Several processes, like the entry it wraps: every pass decision reads reduced norms,
 * so it falls alike on every rank. */
#define PREALPS_REFINE_CONVERGED         0
#define PREALPS_REFINE_OUT_OF_PASSES     1
#define PREALPS_REFINE_OUT_OF_ITERATIONS 2
#define PREALPS_REFINE_STAGNATED         3
int preAlps_ECGSolveSystemRefined(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb,
                                  const double* x0, int ldx0, double* x, int ldx, int flags,
                                  double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb,
                                  double* sys_res, int max_hist, int* n_hist, int max_passes, int* n_passes,
                                  int* pass_iters, double* pass_res, int* status);
/* preAlps_ECGSolveSystem with the energy-norm error estimate per system, and optionally a stopping test on it.
 *   With A-orthonormal directions an iteration is X += P alpha, and it takes exactly delta_j(i) = ||alpha_i 1_{G_j}||^2
 * off ||x*_j - x_j||_A^2 (G_j: the columns of system j).  The norm is the same in the caller's system and in the
 * scaled, permuted one, so no row map and no pass over a panel is needed: one small launch per iteration reads the
 * alpha that the update of X uses, and the host reads its k words with the residual norm.  Several processes: alpha is
 * global behind the Gram all-reduce, so every rank forms the same words and the iteration gains no collective.
 *   The estimate of the error after iteration l, made at iteration n > l, is est_j(l)^2 = sum_{i=l}^{n-1} delta_j(i): a
 * lower bound (Hestenes-Stiefel, with a delay).  Window rule (tau in (0, 0.5), dmin >= 2; 0.1 and 4 are the usual
 * values): l_j(n) = the largest l <= n - dmin whose second half holds at most tau of the window's sum.  Under
 * geometric decay est^2 / true^2 >= 1 - (tau / (1 - tau))^2; the estimate is a heuristic, not a guarantee
 * (prealps_amd/csrc/ecg_energy.h states the rule and its limits).
 *   flags: those of preAlps_ECGSolveSystem, and
 * PREALPS_SYS_ENERGY: form the drops and return the estimates; the stopping test is the one the other flags select, and
 *   x, every history and the iteration count are those of preAlps_ECGSolveSystem, bit for bit;
 * PREALPS_SYS_STOP_ENERGY (implies PREALPS_SYS_ENERGY): the iteration goes on while for some system no window
 *   qualifies or est_j(l_j(n))^2 > tol^2 * sum_{i<n} delta_j(i), the latter a lower bound of ||x*_j - x0_j||_A^2: the test
 *   is relative to the initial error, with or without a guess.  ecg->maxIter, bs > 0 and a NaN stop as ever.
 * Without either bit the entry IS preAlps_ECGSolveSystem (tau and dmin are not looked at, the new outputs not written).
 *   Outputs, any of which may be NULL (leading dimension max_hist, system j): drop_hist[i + j*max_hist] = delta_j(i);
 * err_hist[i + j*max_hist] = the best estimate of ||x*_j - x_j||_A after i iterations that was available when the solve
 * ended, -1 where no window qualified; sys_err[j] = the estimate at the last window that qualified, sharpened by the
 * drops since, and sys_err_iter[j] the iteration it belongs to (-1, and sys_err[j] = -1: none qualified);
 * sys_energy[j] = sqrt(sum_i delta_j(i)).  A guess that already meets the residual threshold comes back after no
 * iteration, as from preAlps_ECGSolveSystem, and the estimates say "none".
 *   ORTHODIR and ORTHOMIN with NO_BS_RED, one system or several, one process or several.  Refused, naming this entry:
 * ADAPT_BS or ORTHODIR_FUSED with an energy flag, PREALPS_SYS_STOP_ENERGY together with PREALPS_SYS_STOP_ORIGINAL, tau
 * or dmin out of range, nrhs > 16, and everything preAlps_ECGSolveSystem refuses.  Statistic "ecg_energy_launches". */
#define PREALPS_SYS_ENERGY      4   /* form the drops, return the estimates */
#define PREALPS_SYS_STOP_ENERGY 8   /* implies 4; refused with PREALPS_SYS_STOP_ORIGINAL */
int preAlps_ECGSolveSystemEnergy(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb,
                                 const double* x0, int ldx0, double* x, int ldx, int flags, double tau, int dmin,
                                 double* res_hist, int* bs_hist, double* sys_hist, double* sys_normb, double* sys_res,
                                 double* drop_hist, double* err_hist, double* sys_err, int* sys_err_iter,
                                 double* sys_energy, int max_hist, int* n_hist);
/* ---- solution history: start a solve from the best mix of earlier solutions ---------------------------------------
 * For a sequence of systems on one operator (a time loop, a Newton loop, a sweep).  The history belongs to the built
 * operator and is process-global like it: Xh, up to capacity <= 16 columns of N doubles on the device, in the caller's
 * order and units (exactly what preAlps_ECGSolveSystem returns; a scaling vector that preAlps_OperatorUpdateValues
 * changes therefore needs no rescaling), kept as a ring -- a full ring evicts its oldest column -- and G = Xh^T A Xh
 * (fp64, on the host, exactly symmetric, with the "op_values_epoch" it was formed at).  x^T A y is the same number in
 * the caller's system and in the scaled, permuted one.
 *   preAlps_SolutionHistoryProject (Fischer's projection): g = Xh^T B; G scaled to unit diagonal; a diagonally pivoted
 * Cholesky that stops when the largest remaining pivot is <= rtol (rtol <= 0: 1e-12); a dropped column gets the
 * coefficient 0 and *rank is the number kept; x0 = Xh c (N x nrhs, ldx0 >= N) is the element of span(Xh) closest to the
 * solution of A x = b in the energy norm, and captured[j] (may be NULL) = c_j^T g_j = ||x0_j||_A^2.  An empty history
 * gives rank 0 and x0 = 0.  Two projections of the same input agree in bits: the dots are folded in a fixed order, no
 * atomics are used.  (prealps_amd/csrc/ecg_history.h states the rule and its limits.)
 *   preAlps_SolutionHistoryAppend: w = A x by the library's own fp64 product -- the gather of (D^-1 x)[perm], a plain
 * product at s = 1 on the fp64 values (as preAlps_OperatorSystemResiduals forms it) -- then the new rows and columns of
 * G from Xh^T w and x^T w, read through the operator's row map, then the columns into the ring; the evicted rows and
 * columns of G are overwritten on the host.  More columns than the capacity: the last `capacity` are kept.
 *   Refresh: at the first project or append after preAlps_OperatorUpdateValues, G is formed again from Xh and the new
 * matrix (one product over the live columns; stat "hist_gram_refreshes").
 *   preAlps_ECGSolveSystemHistory: project, preAlps_ECGSolveSystem from that x0, append the returned x (nothing is
 * appended when the start already met every threshold: *n_hist = 0, no iteration).  With an empty history, or rank 0,
 * it is preAlps_ECGSolveSystem with x0 = NULL bit for bit; otherwise preAlps_ECGSolveSystem with the projected x0 bit
 * for bit.  sys_res0 (may be NULL): the start residuals in the metric of the test; *rank (may be NULL): the columns the
 * projection kept.  Every other argument is preAlps_ECGSolveSystem's.
 *   preAlps_SolutionHistoryCreate(capacity), 1 .. 16, replaces an existing history; preAlps_SolutionHistoryFree (also
 * done by preAlps_OperatorFree; no error without a history); preAlps_SolutionHistoryClear empties the ring.
 *   flags: PREALPS_SYS_DEVICE (the arrays are device pointers, read and written on the library stream) and, for the
 * solve, PREALPS_SYS_STOP_ORIGINAL.  Every entry returns after the library stream has drained.
 *   Stats: "hist_capacity", "hist_columns", "hist_bytes", "hist_appends" (columns), "hist_projections",
 * "hist_last_rank", "hist_gram_refreshes", "hist_values_epoch"; all 0 without a history.
 *   Refused, naming the entry and leaving the history as it was: no operator, no history, a capacity out of range;
 * nrhs < 1 or > 16; a leading dimension below N, a NULL array, a non-finite x or b; plan-only mode;
 * everything preAlps_ECGSolveSystem refuses; a G whose largest diagonal entry is not positive and finite.
 *   Several processes (or a preAlps_hip_loopback shard): the entries are collective.  The ring holds the m rows this
 * process owns ("hist_bytes" = 8 m capacity); b, x and x0 stay the caller's global arrays (N rows, ld >= N) on every
 * process, read and written at the owned rows alone -- the other rows of x0 are left untouched, so x0 buffers that start
 * as zeros sum to the whole start vector.  The local sums of an entry travel in one all-reduce (a projection costs 1,
 * an append and a refresh of G 2 each: the agreement ahead of the distributed product, then the sums), so rank, captured,
 * G and every counter are the same on every process.  A wrong leading dimension, a NULL array or a failed allocation on
 * one process makes every process return nonzero, a NaN or Inf in one process's rows makes every process refuse with
 * the "not finite" message, and the history stays as it was on all of them.  Refused on every process: an operator
 * built for another process group than the current one; more than one process without an all-reduce hook
 * (preAlps_hip_set_comm, preAlps_hip_rccl_init, an MPI launcher). */
int preAlps_SolutionHistoryCreate(int capacity);
int preAlps_SolutionHistoryFree(void);
int preAlps_SolutionHistoryClear(void);
int preAlps_SolutionHistoryAppend(int nrhs, const double* x, int ldx, int flags);
int preAlps_SolutionHistoryProject(int nrhs, const double* b, int ldb, double* x0, int ldx0, int flags, double rtol,
                                   int* rank, double* captured);
int preAlps_ECGSolveSystemHistory(preAlps_ECG_t* ecg, int nrhs, const double* b, int ldb, double* x, int ldx,
                                  int flags, double rtol, double* res_hist, int* bs_hist, double* sys_hist,
                                  double* sys_normb, double* sys_res, double* sys_res0, int* rank, int max_hist,
                                  int* n_hist);
/* 1 / 0: the two driver loops above and below replay each half of an iteration from a HIP graph
 * captured on its first passes (default: off, or PREALPS_ECG_GRAPH; plain launches measured faster). */
void preAlps_hip_graphs(int on);
/* Storage of the sparse (nested-dissection) factors that large diagonal blocks get, from the next
 * preAlps_BlockJacobiCreate on: 64 = fp64; 32 = fp32 (factored in fp64, both panel copies rounded from the
 * same values, every operation of the apply in fp64: half the bytes the block solve streams, a preconditioner
 * that stays exactly symmetric positive definite and loses fp32 rounding in quality); 0 (default) = follow
 * PREALPS_BJ_ND_PRECISION (`double`, the default, or `single`; any other value makes the create fail).  Band
 * blocks -- every block without the sparse factor -- stay fp64 either way.  Other values are refused; needs no GPU. */
int preAlps_hip_set_nd_precision(int bits);
/* Storage of the one-copy band records (the factor that the block solve of panels of up to 4 columns, and of 5 to 8
 * columns when PREALPS_BJ_G4_WIDE allows, reads in both sweeps), from the next preAlps_BlockJacobiCreate on:
 * 64 = fp64; 32 = fp32 (the strictly lower part of L D^-1 rounded once, D^-2 and every operation of the apply in
 * fp64: both sweeps read the same record, so the block solve stays exactly symmetric positive definite; half the
 * bytes those launches stream); 0 (default) = follow PREALPS_BJ_BAND_PRECISION (`double`, the default, or `single`;
 * any other value makes the create fail).  Independent of preAlps_hip_set_nd_precision.  The plain fp64 records
 * that the kernels for 9 to 16 columns and for wide bands read are not touched: those applies keep the fp64 bits.
 * Other values are refused; needs no GPU. */
int preAlps_hip_set_band_precision(int bits);
/* Storage of the matrix values that preAlps_BlockOperator streams: 64 = fp64; 32 = fp32 (every value rounded once,
 * widened again exactly in the kernel, every operation in fp64 in the order of the fp64 kernel: a product has the
 * bits of the fp64 product with the rounded matrix, which stays symmetric and keeps its zeros); 0 (default) = follow
 * PREALPS_SPMM_PRECISION (`double`, the default, or `single`; any other value makes the next plan cut fail and is
 * named there).  Other values are refused; needs no GPU and works in plan-only mode.
 *   It takes effect at once: the library stream is drained and a plan that is on the device gets or drops its fp32
 * copy inside the call.  fp32 reaches the packed run plan at a panel stride of at most 4 columns (k_spmm_runs_pack,
 * k_spmm_runs_gram_pack; with 32 in force a run plan at such a stride is packed whatever that saves, unless
 * PREALPS_SPMM_PACK=0, which wins).  Every other plan -- the window plan, the staged plan, the unpacked run plan, 8 and
 * 16 columns -- keeps its fp64 values and its bits; the stat "spmm_precision" (64 / 32) tells which the plan in use
 * reads.  The fp64 array stays on the device beside the copy and does not move ("spmm_val_address"); the copy is
 * formed again after every plan cut, after preAlps_OperatorUpdateValues (in place when the update writes through;
 * in a new allocation when it packs anew) -- stats "spmm_val32_bytes", "spmm_val32_address",
 * "spmm_precision_stream_bytes" (what one product streams), "spmm_round_kernel_s".
 *   A value that is finite in fp64 and not in fp32 is refused: the copy is freed, the call (or the product that cut
 * the plan, or the update) fails and names the value; a scaled operator has |a'| <= 1 and cannot meet this.
 *   The rounded matrix is another matrix: a solve converges to ITS solution, off by up to cond(A) 2^-24 relative.
 * The product that forms the start residual of a guess (preAlps_ECGInitializeGuess, preAlps_ECGSolveSystem with x0,
 * preAlps_OperatorSystemResiduals) therefore always reads the fp64 values; preAlps_ECGSolveSystemRefined builds on it. */
int preAlps_hip_set_operator_precision(int bits);
/* 1: the two driver loops run an Orthodir iteration of a solver described by the arguments with the block solve
 * before the update of X and R (one finish and one row pass per iteration; bitwise the same results), 0: in the
 * order of preAlps_ECGIterate.  PREALPS_ECG_SOLVE_FIRST=0 (read here as a solver reads it when it is reset) keeps
 * the latter everywhere.  bj_gram / spmm_gram: the block solve / the SpMM can leave the Gram blocks behind. */
int preAlps_hip_ecg_solve_first(int nprocs, int ortho_alg, int bs_red, int enlFac, int fuse, int lazy_norm,
                                int lazy_stop, int bj_gram, int spmm_gram, int graphs);
/* The same loop advanced by nsteps full iterations from the current RCI state,
 * restarting from rhs when the stopping test fires (counts go to the optional
 * out-parameters).  Used for timing a fixed number of iterations. */
int preAlps_ECGAdvance(preAlps_ECG_t* ecg, double* rhs, int* rci_request, int nsteps, int* restarts,
                       int* last_iters, double* last_res);
/* Device panel <-> host column-major array (ld >= m). */
int preAlps_hip_panel_alloc(CPLM_Mat_Dense_t* A, int M, int N, int m, int n, int enlFac);
void preAlps_hip_panel_free(CPLM_Mat_Dense_t* A);
int preAlps_hip_panel_to_host(const CPLM_Mat_Dense_t* A, int enlFac, double* host, int ld);
int preAlps_hip_panel_from_host(CPLM_Mat_Dense_t* A, int enlFac, const double* host, int ld);
/* The tall-skinny panel kernels of the iteration on their own (what a kernel-level check calls;
 * the solver launches the same kernels): host_out (ld_out >= rows) = [A0 | A1]^T B, column major
 * (the dgemm of ecg.c:311,330,347,425,438,510);  Z -= [V0 | V1] beta with beta on the host,
 * column major (ecg.c:354,517);  P <- P U^-1, AP <- AP U^-1, X += P alpha, R -= AP alpha and
 * *host_res2 = sum of squares of the new R (ecg.c:324-338,434-435,500-501,250), U upper
 * triangular t x t, alpha t x X.n, both on the host, column major.  A1 / V1 may be NULL. */
int preAlps_hip_panel_gram(const CPLM_Mat_Dense_t* A0, const CPLM_Mat_Dense_t* A1, const CPLM_Mat_Dense_t* B,
                           double* host_out, int ld_out);
int preAlps_hip_panel_update(CPLM_Mat_Dense_t* Z, const CPLM_Mat_Dense_t* V0, const CPLM_Mat_Dense_t* V1,
                             const double* host_beta, int ldb);
int preAlps_hip_panel_trsm_update(CPLM_Mat_Dense_t* P, CPLM_Mat_Dense_t* AP, CPLM_Mat_Dense_t* X,
                                  CPLM_Mat_Dense_t* R, const double* host_U, const double* host_alpha,
                                  double* host_res2);
/* BF-Omin's second half on its own (ecg.c:358-393): P(:, c) = Z(:, piv[c]), c < Z.n, then the leading t columns
 * times U^-1 (t x t upper triangular, host, column major, piv 0-based on the host); one_pass = the solver's single
 * kernel, 0 = the three kernels it replaces (same bits). */
int preAlps_hip_panel_permute_solve(const CPLM_Mat_Dense_t* Z, CPLM_Mat_Dense_t* P, const int* host_piv, int t,
                                    const double* host_U, int one_pass);
/* Numeric facts about the built operator / preconditioner, by name:
 * "nnz_local", "rows_local", "halo_rows", "spmm_blocks", "bj_factor_bytes" (bytes of block factors
 * stored: the sparse ones at 4 bytes per entry in single precision), "bj_max_bandwidth", "bj_parts_local",
 * "bj_nd_blocks" (blocks with the sparse factor), "bj_nd_inverse_dev" (largest deviation of its inverted
 * pivot triangles), "bj_nd_precision" (64 / 32: storage of the sparse factors, 0: no block has one; band
 * blocks are always fp64 under that switch), "bj_band_precision" (64 / 32: storage of the one-copy band records,
 * 0: no class has them, e.g. PREALPS_BJ_G4=0), "bj_g4_bytes" (bytes of those records as stored: half in single
 * precision; "bj_factor_bytes" does not count them), "bj_g4_last_ring" / "bj_g4_last_bits" /
 * "bj_g4_last_pipelined" (the last launch that read them: LDS ring depth, storage bits of the records, 1 = the
 * pipelined few-blocks chain), "bj_g4_last_paired" (1 = that launch was the PAIR launch: two blocks of one class of
 * identical blocks per wavefront, PREALPS_BJ_PAIR), "bj_pair_tasks" / "bj_paired_blocks" (the pair tasks of the create:
 * wavefronts of the PAIR launch, and the blocks among them that have a partner), "bj_share_classes" / "bj_shared_blocks" / "bj_share_distinct_g4_bytes" (identical
 * diagonal blocks read one block's records, PREALPS_BJ_SHARE: classes found by the create, blocks that read another
 * block's records now -- after preAlps_BlockJacobiUpdateValues those that still do -- and the bytes of the one-copy
 * records that are read at all; "bj_share_s": seconds of the create's class pass), "ecg_graph_captures" / "ecg_graph_replays" (iteration segments captured and graphs
 * launched by the driver loops so far, preAlps_hip_graphs), "ecg_x_skips" / "ecg_x_flushes" (row passes of the
 * library's loops that left X alone so far, and owed updates of X that a stop paid with a launch of its own,
 * PREALPS_ECG_X_DEFER), "ecg_energy_launches" (launches of the energy-norm drops the iteration has queued so far:
 * one per iteration of a solve with PREALPS_SYS_ENERGY / PREALPS_SYS_STOP_ENERGY, none otherwise), "spmm_precision" (64 / 32: storage of the values the plan in use streams, 0: no plan
 * yet), ...  Returns non-zero for unknown keys. */
int preAlps_hip_get_stat(const char* key, double* value);
/* A stopwatch made of two hipEvents on the library stream: start records the
 * first, stop records the second, waits for it and returns the device time
 * between them (what bench.py uses to time a batch of launches). */
int preAlps_hip_timer_start(void);
int preAlps_hip_timer_stop(double* seconds);
/* Streaming ceilings of the device from two calibration kernels (plain copy, plain read) over
 * `bytes` of freshly allocated HBM, `reps` launches each, timed with the stopwatch above. */
int preAlps_hip_hbm_probe(size_t bytes, int reps, double* copy_GBs, double* read_GBs);
/* Per-phase device time in seconds accumulated since the last reset, from
 * hipEvents on the library stream when timing is enabled (it adds a stream
 * sync per call, so it is off by default).  Keys: "operator", "precond",
 * "gram", "trsm", "update", "small", "comm". */
void preAlps_hip_timing(int enable);
void preAlps_hip_timing_reset(void);
int preAlps_hip_get_time(const char* key, double* seconds);

#ifdef __cplusplus
}
#endif
#endif
