"""Host-side mirror of the reference driver (examples/test_ecg_prealps_op.c:151-239)
on top of the C ABI: build the operator, factor the block-Jacobi preconditioner,
run the reverse-communication loop.  Everything numeric happens in
libprealps_hip.so on the GPU; numpy only carries host arrays in and out.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import lib as _l
from .lib import (ADAPT_BS, NO_BS_RED, ORTHODIR, ORTHODIR_FUSED, ORTHOMIN, CPLM_Mat_CSR_t,
                  CPLM_Mat_Dense_t, check, preAlps_ECG_t)


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@dataclass
class EcgResult:
    x: np.ndarray
    iters: int
    res: np.ndarray          # residual norm after every stopping test
    bs: np.ndarray           # block size after every stopping test
    final_res: float
    final_bs: int
    normb: float
    seconds: float = 0.0
    timers: dict = field(default_factory=dict)
    # solve_multi only: g_j at the stop, ||b_j||, and g_j after every stopping test (iterations x systems)
    sys_res: np.ndarray = None
    sys_normb: np.ndarray = None
    sys_hist: np.ndarray = None
    # a solve from an initial guess (x0= / X0=): the residual norm every system starts from
    sys_res0: np.ndarray = None
    # solve_system only: the metric of the stopping test, of sys_res, sys_normb and sys_hist ("original" / "scaled"),
    # and the recurrence residual norms ||b_j - A x_j|| in the caller's units at the end, whichever metric stopped it
    metric: str = None
    sys_res_original: np.ndarray = None
    # solve_system(refine=True) only: the passes that iterated, the iterations of each, the start residuals of every
    # pass in the metric of the stopping test (row p; row `passes` = what ended the chain), and why it ended:
    # "converged", "out of passes", "out of iterations" or "stagnated"
    passes: int = None
    pass_iters: np.ndarray = None
    pass_res: np.ndarray = None
    refine_status: str = None
    # solve_system(stop="energy") / solve_system(energy=True) only: delta_j(i), the squared energy-norm drop of every
    # iteration (iterations x systems); err_hist[i, j], the best estimate of ||x*_j - x_j||_A after i iterations that was
    # available at the end (iterations + 1 rows, -1 where no window qualified); err_est[j] / err_iter[j], the estimate
    # at the last window that qualified and the iteration it belongs to (-1: none); energy_norm[j] = sqrt(sum_i delta_j(i)),
    # a lower bound of ||x*_j - x0_j||_A
    drop_hist: np.ndarray = None
    err_hist: np.ndarray = None
    err_est: np.ndarray = None
    err_iter: np.ndarray = None
    energy_norm: np.ndarray = None
    # solve_system(history=True) (preAlps_ECGSolveSystemHistory): the columns of the history the projection kept, and
    # the start residuals of the projected start in the metric of the test (||b_j|| where nothing was kept)
    history_rank: int = None
    sys_res0: np.ndarray = None


class DistributedHooks:
    """Binds the library's two communication hooks to torch.distributed.

    backend "nccl" is RCCL on ROCm: the device buffers are wrapped zero-copy as
    torch tensors and reduced / exchanged in place.  With "gloo" (CPU tests and
    single-GPU rehearsals) the buffers are staged through host memory.
    """

    def __init__(self, L):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.L = torch, dist, L
        self.rank, self.size = dist.get_rank(), dist.get_world_size()
        self.staged = dist.get_backend() != "nccl"
        # everything the hooks do is queued on the library's own stream, so it is ordered
        # after the kernels that produced the buffers and before the ones that consume them
        self._streams = {}
        self._ar = _l.ALLREDUCE_FN(self._allreduce)
        self._ex = _l.EXCHANGE_FN(self._exchange)
        check(L.preAlps_hip_set_world(self.rank, self.size), "preAlps_hip_set_world")
        check(L.preAlps_hip_set_comm(self._ar, self._ex, None), "preAlps_hip_set_comm")

    def _stream(self):
        # the library switches to its side stream around the halo exchange
        h = int(self.L.preAlps_hip_get_stream())
        st = self._streams.get(h)
        if st is None:
            st = self._streams[h] = self.torch.cuda.ExternalStream(h)
        return st

    def _wrap(self, ptr, count):
        """Zero-copy float64 view of `count` doubles of device memory owned by the library."""
        torch = self.torch
        dev = torch.device("cuda", torch.cuda.current_device())
        st = torch._C._construct_storage_from_data_pointer(int(ptr), dev, 8 * int(count))
        t = torch.empty(0, dtype=torch.float64, device=dev).set_(st, 0, (int(count),), (1,))
        if t.data_ptr() != int(ptr):
            raise RuntimeError("could not alias library memory as a torch tensor")
        return t

    def _allreduce(self, ctx, ptr, count):
        try:
            with self.torch.cuda.stream(self._stream()):
                t = self._wrap(ptr, count)
                if self.staged:
                    h = t.cpu()
                    self.dist.all_reduce(h)
                    t.copy_(h)
                else:
                    self.dist.all_reduce(t)
            return 0
        except Exception as e:  # pragma: no cover - surfaced through the C error path
            print("all-reduce hook failed:", e)
            return 1

    def _exchange(self, ctx, send, send_counts, recv, recv_counts, peers, npeers):
        try:
            dist, torch = self.dist, self.torch
            ns = sum(send_counts[i] for i in range(npeers))
            nr = sum(recv_counts[i] for i in range(npeers))
            with torch.cuda.stream(self._stream()):
                ts_ = self._wrap(send, max(ns, 1))
                tr_ = self._wrap(recv, max(nr, 1))
                if self.staged:
                    hs, hr = ts_.cpu(), torch.empty(max(nr, 1), dtype=torch.float64)
                else:
                    hs, hr = ts_, tr_
                ops, so, ro = [], 0, 0
                for i in range(npeers):
                    p, sc, rc = peers[i], send_counts[i], recv_counts[i]
                    if sc:
                        ops.append(dist.P2POp(dist.isend, hs[so:so + sc], p))
                    if rc:
                        ops.append(dist.P2POp(dist.irecv, hr[ro:ro + rc], p))
                    so += sc
                    ro += rc
                for w in dist.batch_isend_irecv(ops) if ops else []:
                    w.wait()
                if self.staged and nr:
                    tr_[:nr].copy_(hr[:nr])
            return 0
        except Exception as e:  # pragma: no cover
            print("halo-exchange hook failed:", e)
            return 1


def bind_process_group(L, prefer=None):
    """Install the communication hooks of this process for the current torch.distributed
    group.  With the "nccl" backend the library's own RCCL binding is used (C, on the
    library stream: no host round trip); the torch.distributed hooks are the fallback
    and what "gloo" uses.  Returns (kind, keep_alive_object)."""
    import os
    import ctypes as C
    import torch.distributed as dist
    prefer = prefer or os.environ.get("PREALPS_COMM", "rccl")
    rank, size = dist.get_rank(), dist.get_world_size()
    if prefer == "rccl" and dist.get_backend() == "nccl":
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())

        def all_ok(ok):
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            return int(flag.item()) == 1

        # vote BEFORE the collective ncclCommInitRank: a rank that cannot load librccl or (rank 0)
        # cannot create the id must not leave the others blocked inside it
        buf = C.create_string_buffer(128)
        ok = L.preAlps_hip_rccl_available() == 0
        if ok and rank == 0:
            ok = L.preAlps_hip_rccl_unique_id(buf) == 0
        if not ok:
            print("[prealps_amd] native RCCL hooks unavailable on rank %d (%s)" % (rank, L.preAlps_hip_last_error()))
        if all_ok(ok):
            box = [bytes(buf.raw)]
            dist.broadcast_object_list(box, src=0)
            ok = L.preAlps_hip_rccl_init(box[0], rank, size) == 0
            ok = ok and L.preAlps_hip_comm_selftest() == 0
            if not ok:
                print("[prealps_amd] native RCCL binding failed on rank %d (%s)" % (rank, L.preAlps_hip_last_error()))
            # every rank must end up on the same binding: one failure sends all of them to the fallback
            if all_ok(ok):
                return "rccl", None
        if rank == 0:
            print("[prealps_amd] using the torch.distributed hooks on all ranks")
    hooks = DistributedHooks(L)
    check(L.preAlps_hip_comm_selftest(), "preAlps_hip_comm_selftest")
    return "torch." + dist.get_backend(), hooks


def partition_kway(rowptr, colind, nparts):
    """preAlps_hip_partition_kway: the library's stand-in for METIS_PartGraphKway (host code)."""
    L = _l.load()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colind = np.ascontiguousarray(colind, dtype=np.int32)
    part = np.empty(len(rowptr) - 1, dtype=np.int32)
    check(L.preAlps_hip_partition_kway(len(part), _pi(rowptr), _pi(colind), int(nparts), _pi(part)),
          "preAlps_hip_partition_kway")
    return part


class EcgProblem:
    """One operator + one block-Jacobi preconditioner (both process-global in
    the library, as in the reference) and solves on them."""

    def __init__(self, rowptr, colind, val, nparts, part=None, scale=True, device=None,
                 distributed=False, use_torch_stream=False, partitioner=False, shard=None, plan_only=False):
        """part: explicit partition vector; None = contiguous row blocks, or -- with
        partitioner=True -- the library's k-way graph partitioner (what preAlps_OperatorBuild
        uses where the reference calls METIS).  shard = (r, G): rehearse rank r of a G-process run in
        this one process (preAlps_hip_loopback).  plan_only=True: the host side alone, without a GPU
        (preAlps_hip_plan_only, until close()): the panel, the halo plan and update_values work, products and
        solves are refused."""
        self.L = L = _l.load()
        import os
        dev = int(os.environ.get("LOCAL_RANK", "0")) if device is None else device
        self._plan_only = bool(plan_only)
        if self._plan_only:
            L.preAlps_hip_plan_only(1)
        else:
            check(L.preAlps_hip_init(dev), "preAlps_hip_init")
        self.hooks, self.comm_kind = None, "none"
        if distributed:
            import torch
            torch.cuda.set_device(dev)
            self.comm_kind, self.hooks = bind_process_group(L)
        if shard is not None:
            check(L.preAlps_hip_loopback(int(shard[0]), int(shard[1])), "preAlps_hip_loopback")
            self.comm_kind = "loopback %d/%d" % (shard[0], shard[1])
        if use_torch_stream:
            import torch
            check(L.preAlps_hip_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "preAlps_hip_set_stream")
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colind = np.ascontiguousarray(colind, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        self.N = len(rowptr) - 1
        self._nnz_global = int(rowptr[-1])
        p = None if part is None else np.ascontiguousarray(part, dtype=np.int32)
        if p is None and partitioner:
            p = partition_kway(rowptr, colind, nparts)
        rc = L.preAlps_OperatorBuildFromCSR(self.N, _pi(rowptr), _pi(colind), _pd(val), int(nparts),
                                            None if p is None else _pi(p), 1 if scale else 0)
        if rc != 0 and self._plan_only:
            L.preAlps_hip_plan_only(0)
        check(rc, "preAlps_OperatorBuildFromCSR")
        self._after_build()

    @classmethod
    def from_mtx(cls, path, nparts=None, device=0, partition=None):
        """preAlps_OperatorBuild(file, comm) like the reference driver.  partition: None = the
        library's graph partitioner (where the reference calls METIS), "contiguous" = row blocks."""
        import os
        self = cls.__new__(cls)
        self.L = L = _l.load()
        self.hooks, self.comm_kind = None, "none"
        self._plan_only = False
        check(L.preAlps_hip_init(device), "preAlps_hip_init")
        if nparts is not None:
            os.environ["PREALPS_NPARTS"] = str(nparts)
        if partition is None:
            os.environ.pop("PREALPS_PARTITION", None)
        else:
            os.environ["PREALPS_PARTITION"] = partition
        check(L.preAlps_OperatorBuild(path.encode(), 0x44000000), "preAlps_OperatorBuild")
        self._after_build()
        return self

    def _after_build(self):
        L = self.L
        M, m = C.c_int(), C.c_int()
        check(L.preAlps_OperatorGetSizes(C.byref(M), C.byref(m)), "preAlps_OperatorGetSizes")
        self.M, self.m = M.value, m.value
        self.N = self.M
        self.A = CPLM_Mat_CSR_t()
        check(L.preAlps_OperatorGetA(C.byref(self.A)), "preAlps_OperatorGetA")
        rp, n = C.POINTER(C.c_int)(), C.c_int()
        check(L.preAlps_OperatorGetRowPosPtr(C.byref(rp), C.byref(n)), "preAlps_OperatorGetRowPosPtr")
        self._rowpos_ptr, self._rowpos_n = rp, n.value
        self.rowpos = np.ctypeslib.as_array(rp, shape=(n.value,)).copy()
        cp, cn = C.POINTER(C.c_int)(), C.c_int()
        check(L.preAlps_OperatorGetColPosPtr(C.byref(cp), C.byref(cn)), "preAlps_OperatorGetColPosPtr")
        self._colpos_ptr, self._colpos_n = cp, cn.value
        pp, pn = C.POINTER(C.c_int)(), C.c_int()
        check(L.preAlps_OperatorGetPermPtr(C.byref(pp), C.byref(pn)), "preAlps_OperatorGetPermPtr")
        self.perm = np.ctypeslib.as_array(pp, shape=(pn.value,)).copy()
        self.nparts = L.preAlps_hip_nparts()
        self.row_off = 0
        self.has_precond = False
        self._precond_args = (None, None)
        self._coarse = None
        self._set_precision = False

    def part_vector(self):
        """part[i] of every original row i, recovered from the permutation and rowPos."""
        part = np.empty(self.N, dtype=np.int32)
        part[self.perm] = np.repeat(np.arange(self.nparts, dtype=np.int32), np.diff(self.rowpos))
        return part

    # -- pieces of the driver --------------------------------------------------
    def set_coarse_space(self, V, aggregates=None):
        """preAlps_BlockJacobiSetCoarseSpace: M^-1 = B^-1 + Z E^-1 Z^T from the k columns of V (N x k, or N values
        for one vector; 1 <= k <= 8), given in the order and units of the matrix this problem was built from
        (nearkernel.translations, nearkernel.rigid_body_modes).  aggregates: one aggregate id per part (numbered
        0 .. naggr - 1, none empty); None = one aggregate per part when that fits stat("bj_coarse_max_dofs"),
        otherwise the library's partition of the parts' quotient graph.  Creates the block-Jacobi factor first if
        there is none.  A refusal raises and leaves the preconditioner (and an earlier coarse space) as it was.
        On a distributed=True problem the call is collective: every rank passes the same GLOBAL V (all N rows) and the
        same global aggregates (one id per part of ALL ranks, an aggregate may span ranks; None: no default aggregate
        spans ranks, and over the cap every rank cuts the quotient graph of its own parts).  Every rank keeps only what
        its own rows need, an apply costs one all-reduce more, and what one rank alone refuses (a NaN in its copy of V)
        raises on every rank.  A shard= problem refuses."""
        V = np.asarray(V, dtype=np.float64)
        if V.ndim == 1:
            V = V[:, None]
        if V.ndim != 2:
            raise ValueError("V must be two-dimensional (N x k), not of shape %r" % (V.shape,))
        if V.shape[0] != self.N:
            raise ValueError("V has %d rows, the matrix has %d" % (V.shape[0], self.N))
        V = np.asfortranarray(V)
        agg, naggr = None, 0
        if aggregates is not None:
            agg = np.ascontiguousarray(aggregates, dtype=np.int32)
            if agg.shape != (self.nparts,):
                raise ValueError("aggregates must hold one id per part (%d), not be of shape %r" % (self.nparts, agg.shape))
            naggr = int(agg.max()) + 1 if agg.size else 0
        if not self.has_precond and not self._plan_only:
            self.create_block_jacobi()
        check(self.L.preAlps_BlockJacobiSetCoarseSpace(int(V.shape[1]), _pd(V), max(self.N, 1),
                                                       None if agg is None else _pi(agg), naggr),
              "preAlps_BlockJacobiSetCoarseSpace")
        # remembered for update_values(..., precond="rebuild"); V is not copied a second time (the library keeps its
        # own copy): an N x k float64 array in column-major order is held as it is, so leave it unchanged meanwhile
        self._coarse = (V, None if agg is None else agg.copy())

    def coarse_aggregates(self):
        """preAlps_BlockJacobiGetCoarseAggregates: the aggregate of every part of the attached coarse space (the
        ones given, or the default the library chose) as an int32 array of nparts values -- on a distributed problem
        the parts of all ranks, the same array on every rank."""
        agg, n = np.zeros(self.nparts, dtype=np.int32), C.c_int()
        check(self.L.preAlps_BlockJacobiGetCoarseAggregates(_pi(agg), C.byref(n)), "preAlps_BlockJacobiGetCoarseAggregates")
        return agg

    def clear_coarse_space(self):
        """preAlps_BlockJacobiClearCoarseSpace: plain block Jacobi again, with the bits it had before.  On a distributed
        problem every rank must call it before the next apply or solve (the ranks' applies must launch alike)."""
        check(self.L.preAlps_BlockJacobiClearCoarseSpace(), "preAlps_BlockJacobiClearCoarseSpace")
        self._coarse = None

    def create_block_jacobi(self, nd_precision=None, band_precision=None, coarse=None):
        """coarse: vectors for set_coarse_space(coarse) right after the create (default aggregates; on a distributed
        problem the global N x k array, the same on every rank, and the call is collective).
        nd_precision: storage of the sparse factors of large blocks -- None follows
        PREALPS_BJ_ND_PRECISION, "double" / "single" select it for this create (band blocks stay fp64).
        With a value, the library's setting (preAlps_hip_set_nd_precision) is 0 again afterwards: a value
        set earlier through the C entry is not restored.
        band_precision: the same for the one-copy band records that panels of up to 4 (8) columns read
        (PREALPS_BJ_BAND_PRECISION, preAlps_hip_set_band_precision); the two are independent."""
        bits = {None: 0, "double": 64, "single": 32}.get(nd_precision)
        if bits is None:
            raise ValueError("nd_precision must be None, 'double' or 'single', not %r" % (nd_precision,))
        bbits = {None: 0, "double": 64, "single": 32}.get(band_precision)
        if bbits is None:
            raise ValueError("band_precision must be None, 'double' or 'single', not %r" % (band_precision,))
        if bits:
            check(self.L.preAlps_hip_set_nd_precision(bits), "preAlps_hip_set_nd_precision")
        try:
            if bbits:
                check(self.L.preAlps_hip_set_band_precision(bbits), "preAlps_hip_set_band_precision")
            check(self.L.preAlps_BlockJacobiCreate(C.byref(self.A), self._rowpos_ptr, self._rowpos_n,
                                                   self._colpos_ptr, self._colpos_n),
                  "preAlps_BlockJacobiCreate")
        finally:
            if bits:
                self.L.preAlps_hip_set_nd_precision(0)
            if bbits:
                self.L.preAlps_hip_set_band_precision(0)
        self.has_precond = True
        self._precond_args = (nd_precision, band_precision)
        self._coarse = None                      # (a create frees the old preconditioner with its coarse space)
        if coarse is not None:
            self.set_coarse_space(coarse)

    def refactor_block_jacobi(self):
        """preAlps_BlockJacobiUpdateValues: the factor of the current panel in place -- for band blocks the bits of
        a fresh create_block_jacobi with the precision of the last one, at the same device addresses, without the
        orders, the host assembly and the band upload; blocks with the sparse factor are created again.  A panel
        that is no longer SPD raises and leaves no preconditioner (has_precond becomes False)."""
        rc = self.L.preAlps_BlockJacobiUpdateValues()
        if rc != 0:
            self.has_precond = self.stat("bj_parts_local") > 0     # (freed by the library when the values are not SPD)
            if self.stat("bj_coarse_dofs") == 0:                    # (or only the coarse space dropped: singular E)
                self._coarse = None
        check(rc, "preAlps_BlockJacobiUpdateValues")

    def set_operator_precision(self, precision):
        """preAlps_hip_set_operator_precision: storage of the matrix values the products stream, "double" or "single"
        (every value rounded once to fp32, all arithmetic in fp64).  It takes effect at once and for every plan cut
        later; it reaches the packed run plan at up to 4 columns, every other plan keeps fp64 -- stat("spmm_precision")
        tells.  The setting is the library's: close() of a problem that called this puts it back to the default
        (PREALPS_SPMM_PRECISION); a problem that never did leaves the library's setting alone.  A solve
        on the rounded matrix converges to that matrix's solution; solve_system(..., refine=True) repairs it."""
        bits = {"double": 64, "single": 32}.get(precision)
        if bits is None:
            raise ValueError("precision must be 'double' or 'single', not %r" % (precision,))
        check(self.L.preAlps_hip_set_operator_precision(bits), "preAlps_hip_set_operator_precision")
        self._set_precision = True

    def update_values(self, val, precond="keep"):
        """preAlps_OperatorUpdateValues: new values for the same pattern, partition and scaling flag, in the order of
        the val this problem was built from (the whole matrix); the operator becomes the one a fresh problem built from
        them would hold, bit for bit, without the set-up.  self.A and local_csr() show the new panel.
        precond="keep": the block-Jacobi factor of the old values stays, a lagged preconditioner for the new matrix
        (stat("bj_values_epoch") < stat("op_values_epoch") tells); "rebuild": it is freed and created again from the
        new panel with the precision arguments of the last create_block_jacobi; "refactor": refactor_block_jacobi(),
        the same factor in place.  Without a preconditioner "rebuild" and "refactor" do what "keep" does.
        A coarse space (set_coarse_space) goes along: lagged with the factor under "keep", formed again in place at
        the same device addresses under "refactor", attached again to the new factor under "rebuild"."""
        if precond not in ("keep", "rebuild", "refactor"):
            raise ValueError("precond must be 'keep', 'rebuild' or 'refactor', not %r" % (precond,))
        if val is None:
            ptr = None
        else:
            val = np.ascontiguousarray(val, dtype=np.float64)
            if val.ndim != 1:
                raise ValueError("val must be one-dimensional, not of shape %r" % (val.shape,))
            nnz = getattr(self, "_nnz_global", None)      # (from_mtx: the library refuses, with its own message)
            if nnz is not None and val.shape[0] != nnz:
                raise ValueError("val has %d entries, the matrix this problem was built from has %d"
                                 % (val.shape[0], nnz))
            ptr = _pd(val)
        check(self.L.preAlps_OperatorUpdateValues(ptr), "preAlps_OperatorUpdateValues")
        if precond == "rebuild" and self.has_precond:
            coarse = self._coarse
            self.L.preAlps_BlockJacobiFree()
            self.has_precond = False
            self.create_block_jacobi(*self._precond_args)
            if coarse is not None:                   # the remembered coarse space, attached again to the new factor
                self.set_coarse_space(coarse[0], coarse[1])
        elif precond == "refactor" and self.has_precond:
            self.refactor_block_jacobi()

    @property
    def scaling(self):
        """preAlps_OperatorGetScalingPtr: a NumPy copy of d (N values, entry i for row i of the matrix this problem
        was built from; d_i = sqrt(1 / max_j |a_ij|)), None when the problem is unscaled.  The operator the solver
        iterates on is P D A D P^T with perm[new] = old."""
        d, n = C.POINTER(C.c_double)(), C.c_int()
        check(self.L.preAlps_OperatorGetScalingPtr(C.byref(d), C.byref(n)), "preAlps_OperatorGetScalingPtr")
        if not d:
            return None
        return np.ctypeslib.as_array(d, shape=(n.value,)).copy()

    @property
    def owned_rows(self):
        """preAlps_OperatorGetOwnedRows: a NumPy copy of the caller's rows this process owns, perm[row_off : row_off + m],
        in the operator's local order.  One process: the whole permutation; the ranks' slices partition 0 .. N-1."""
        rows, m = C.POINTER(C.c_int)(), C.c_int()
        check(self.L.preAlps_OperatorGetOwnedRows(C.byref(rows), C.byref(m)), "preAlps_OperatorGetOwnedRows")
        if m.value == 0:
            return np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(rows, shape=(m.value,)).copy()

    def _system_args(self, what, b, x0, x0_name):
        """The checks solve_system and system_residuals share, before any library call: ("host" | "device", k, one
        column given as a vector).  Raises ValueError."""
        def is_tensor(a):
            return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")
        arrays = [("b" if what == "solve_system" else "X" if what == "history_append" else "B", b)] + ([] if x0 is None else [(x0_name, x0)])
        kinds = {"device" if (is_tensor(a) and a.is_cuda) else "host" for _, a in arrays}
        if len(kinds) > 1:
            raise ValueError("%s: host and device arguments are mixed (%s): pass NumPy arrays or float64 CUDA tensors, "
                             "not both" % (what, ", ".join("%s on the %s" % (n, "device" if is_tensor(a) and a.is_cuda
                                                                             else "host") for n, a in arrays)))
        kind = kinds.pop()
        shapes = []
        for name, a in arrays:
            if is_tensor(a):
                import torch
                if a.dtype != torch.float64:
                    raise ValueError("%s: %s has dtype %s, float64 is needed" % (what, name, a.dtype))
                if not a.is_cuda:
                    raise ValueError("%s: %s is a CPU tensor: pass a NumPy array or a CUDA tensor" % (what, name))
            shp = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
            if len(shp) not in (1, 2) or shp[0] != self.N or (len(shp) == 2 and shp[1] < 1):
                raise ValueError("%s: %s must be of shape (%d,) or (%d, k), not %r" % (what, name, self.N, self.N, shp))
            shapes.append(shp)
        if len(shapes) == 2 and shapes[0] != shapes[1]:
            raise ValueError("%s: %s has shape %r, %s has %r" % (what, arrays[1][0], shapes[1], arrays[0][0], shapes[0]))
        return kind, (1 if len(shapes[0]) == 1 else int(shapes[0][1])), len(shapes[0]) == 1

    def _device_columns(self, a):
        """(tensor to keep alive, address, leading dimension) of an (N, k) float64 CUDA tensor: passed as it lies when
        its strides are (1, ld) with ld >= N, otherwise copied once on the device into that layout."""
        import torch
        if a.dim() == 1:
            a = a.unsqueeze(1)
        k = a.shape[1]
        ok = a.stride(0) == 1 and (k == 1 or a.stride(1) >= self.N)
        if not ok:
            a = torch.empty((k, self.N), dtype=torch.float64, device=a.device).copy_(a.t()).t()
        return a, a.data_ptr(), (int(a.stride(1)) if k > 1 else max(self.N, 1))

    def _order_torch_stream(self):
        """The library reads and writes device arguments on its own stream: unless that is torch's current stream
        (use_torch_stream), what torch has queued must be done first."""
        import torch
        cur = torch.cuda.current_stream().cuda_stream
        if int(self.L.preAlps_hip_get_stream() or 0) != int(cur):
            torch.cuda.current_stream().synchronize()

    def solve_system(self, b, t, x0=None, stop="original", ortho_alg=ORTHODIR, bs_red=NO_BS_RED, tol=1e-5,
                     max_iter=1000, refine=False, max_passes=4, energy=False, tau=0.1, dmin=4, history=False,
                     history_rtol=None):
        """preAlps_ECGSolveSystem: A x = b as the caller stated it -- the rows in the order of the matrix this problem
        was built from, the values in its units -- for one system (b of shape (N,)) or k systems (b of shape (N, k), t a
        multiple of k), with or without a starting value x0 of the same shape.
        On a distributed=True or shard= problem the call is collective and b, x0 and x keep that global shape on every
        rank: a rank reads the rows it owns (owned_rows) and the result's x holds them, with zeros in every other row, so
        a SUM all-reduce of x over the ranks is the whole solution; iters, res, normb, sys_res, sys_normb and sys_hist are
        global and the same on every rank.
        stop="original" (the default: this method exists so that tol means the caller's): iterate until
        ||b_j - A x_j|| <= tol * ||b_j|| for every j, both norms in the caller's units; "scaled": the library's own test
        on the scaled system, as solve / solve_multi apply it -- then the iterate is theirs bit for bit.
        NumPy arrays go the host way.  float64 torch CUDA tensors go the device way: they are passed by address (copied
        once on the device if their strides are not (1, ld >= N)), never written, and the result's x is a CUDA tensor;
        unless the problem runs on torch's stream, torch's current stream is synchronised before the call.
        Returns an EcgResult: x in the caller's order and units, metric = stop, sys_res / sys_normb / sys_hist in that
        metric, sys_res_original = the recurrence residual norms in the caller's units at the end; res / bs / normb /
        final_res stay the scaled Frobenius norms.  Mixed host and device arguments, a tensor that is not float64, wrong
        shapes and a bad stop raise ValueError before any library call.
        refine=True: preAlps_ECGSolveSystemRefined -- the same solve, then up to max_passes - 1 more, each started from
        the x before it with a start residual formed on the fp64 matrix, until that residual meets tol (what makes
        set_operator_precision("single") safe); max_iter bounds all passes together, iters is their sum, the histories
        are concatenated, and passes / pass_iters / pass_res / refine_status say what happened.  refine=False is
        preAlps_ECGSolveSystem, and max_passes is not looked at.
        stop="energy" (preAlps_ECGSolveSystemEnergy): iterate until, for every system, the estimate of the energy-norm
        error ||x*_j - x_j||_A -- a delayed lower bound summed from the drops ||alpha 1_{G_j}||^2 of the iterations, window
        rule tau / dmin -- is at most tol times the same bound of the initial error ||x*_j - x0_j||_A.  The estimate is a
        heuristic, not a guarantee.  energy=True forms the drops and the estimates under any stop, at one small launch
        per iteration and without changing a bit of x or of the histories.  Either way the result gains drop_hist,
        err_hist, err_est, err_iter and energy_norm; sys_res / sys_hist are then in the scaled metric under stop="energy".
        Not with refine=True.
        history=True (preAlps_ECGSolveSystemHistory; enable_history first): the solve starts from the projection of the
        solution onto the span of the solutions in the history -- the closest element in the energy norm -- and its x
        is appended afterwards; the result gains history_rank and sys_res0.  With an empty history it is this method
        without x0 bit for bit, otherwise this method with x0 = history_project(b)[0] bit for bit (on a distributed=True
        or shard= problem: collective, on the same ranks, with x0 = the SUM all-reduce of history_project(b)[0]; the
        history holds the rows each rank owns, history_rank is the same on every rank).  Not together with x0=,
        refine=True or the energy estimate: ValueError."""
        if history and (x0 is not None or refine or energy or stop == "energy"):
            raise ValueError("solve_system: history=True takes its start from the history and runs the plain solve: not "
                             "together with x0=, refine=True, energy=True or stop='energy'")
        if stop not in ("original", "scaled", "energy"):
            raise ValueError("stop must be 'original', 'scaled' or 'energy', not %r" % (stop,))
        energy = bool(energy) or stop == "energy"
        if energy and refine:
            raise ValueError("solve_system: the energy-norm estimate is not formed across the passes of refine=True")
        kind, k, vector = self._system_args("solve_system", b, x0, "x0")
        if int(t) < 1 or int(t) % k != 0:
            raise ValueError("the enlarging factor t = %d is not a multiple of the %d right-hand sides" % (t, k))
        if not self.has_precond:
            self.create_block_jacobi()
        import time
        L = self.L
        check(L.preAlps_hip_prepare_operator(int(t)), "preAlps_hip_prepare_operator")
        e = self.new_ecg(t, ortho_alg, bs_red, tol, max_iter)
        flags = _l.SYS_STOP_ORIGINAL if stop == "original" else 0
        N = self.N
        if kind == "device":
            import torch
            flags |= _l.SYS_DEVICE
            bk, pb, ldb = self._device_columns(b)
            xk, px0, ldx0 = (None, None, 0) if x0 is None else self._device_columns(x0)
            # strides (1, N); several ranks: zeros in the rows this rank does not own
            alloc = torch.zeros if self.comm_kind != "none" else torch.empty
            x = alloc((k, N), dtype=torch.float64, device=bk.device).t()
            px, ldx = x.data_ptr(), max(N, 1)
            self._order_torch_stream()
        else:
            bk = np.asfortranarray(np.asarray(b, dtype=np.float64).reshape(N, k))
            pb, ldb = bk.ctypes.data, max(N, 1)
            xk = None if x0 is None else np.asfortranarray(np.asarray(x0, dtype=np.float64).reshape(N, k))
            px0, ldx0 = (None, 0) if xk is None else (xk.ctypes.data, max(N, 1))
            x = np.zeros((N, k), order="F")
            px, ldx = x.ctypes.data, max(N, 1)
        cap = max_iter + 2
        res = np.zeros(cap)
        bs = np.zeros(cap, dtype=np.int32)
        sys_hist = np.zeros((cap, k), order="F")
        sys_normb, sys_end = np.zeros(k), np.zeros(k)
        nh = C.c_int()
        extra = {}
        t0 = time.perf_counter()
        if refine:
            mp = int(max_passes)
            room = max(mp, 0)
            npass, status = C.c_int(), C.c_int()
            pass_iters = np.zeros(room + 1, dtype=np.int32)
            pass_res = np.zeros((room + 1, k))
            check(L.preAlps_ECGSolveSystemRefined(C.byref(e), k, pb, ldb, px0, ldx0, px, ldx, flags, _pd(res), _pi(bs),
                                                  _pd(sys_hist), _pd(sys_normb), _pd(sys_end), cap, C.byref(nh), mp,
                                                  C.byref(npass), _pi(pass_iters), _pd(pass_res), C.byref(status)),
                  "preAlps_ECGSolveSystemRefined")
            extra = dict(passes=npass.value, pass_iters=pass_iters[:npass.value].copy(),
                         pass_res=pass_res[:npass.value + 1].copy(), refine_status=_l.REFINE_STATUS[status.value])
        elif energy:
            drops = np.zeros((cap, k), order="F")
            errs = np.zeros((cap, k), order="F")
            err_est, err_iter, e_norm = np.zeros(k), np.zeros(k, dtype=np.int32), np.zeros(k)
            flags |= _l.SYS_STOP_ENERGY if stop == "energy" else _l.SYS_ENERGY
            check(L.preAlps_ECGSolveSystemEnergy(C.byref(e), k, pb, ldb, px0, ldx0, px, ldx, flags, float(tau), int(dmin),
                                                 _pd(res), _pi(bs), _pd(sys_hist), _pd(sys_normb), _pd(sys_end),
                                                 _pd(drops), _pd(errs), _pd(err_est), _pi(err_iter), _pd(e_norm), cap,
                                                 C.byref(nh)),
                  "preAlps_ECGSolveSystemEnergy")
            n_ = nh.value
            extra = dict(drop_hist=np.ascontiguousarray(drops[:n_]),
                         err_hist=np.ascontiguousarray(errs[:n_ + 1]),
                         err_est=err_est, err_iter=err_iter, energy_norm=e_norm)
        elif history:
            rank, res0 = C.c_int(), np.zeros(k)
            check(L.preAlps_ECGSolveSystemHistory(C.byref(e), k, pb, ldb, px, ldx, flags,
                                                  0.0 if history_rtol is None else float(history_rtol), _pd(res), _pi(bs),
                                                  _pd(sys_hist), _pd(sys_normb), _pd(sys_end), _pd(res0), C.byref(rank),
                                                  cap, C.byref(nh)),
                  "preAlps_ECGSolveSystemHistory")
            extra = dict(history_rank=rank.value, sys_res0=res0)
        else:
            check(L.preAlps_ECGSolveSystem(C.byref(e), k, pb, ldb, px0, ldx0, px, ldx, flags, _pd(res), _pi(bs),
                                           _pd(sys_hist), _pd(sys_normb), _pd(sys_end), cap, C.byref(nh)),
                  "preAlps_ECGSolveSystem")
        dt = time.perf_counter() - t0
        n = nh.value
        if vector:
            x = x[:, 0].contiguous() if kind == "device" else np.ascontiguousarray(x[:, 0])
        timers = {k_: getattr(e, k_) for k_ in ("tot_t", "comm_t", "trsm_t", "gemm_t", "potrf_t", "copy_t")}
        return EcgResult(x=x, iters=e.iter, res=res[:n].copy(), bs=bs[:n].copy(), final_res=e.res, final_bs=e.bs,
                         normb=e.normb, seconds=dt, timers=timers,
                         sys_res=sys_hist[n - 1].copy() if n else (sys_end.copy() if stop == "original" else None),
                         sys_normb=sys_normb, sys_hist=np.ascontiguousarray(sys_hist[:n]), metric=stop,
                         sys_res_original=sys_end, **extra)

    def system_residuals(self, B, X):
        """preAlps_OperatorSystemResiduals: (res, normb) with res[j] = ||b_j - A x_j|| and normb[j] = ||b_j|| in the
        caller's order and units, formed afresh from B and X (shape (N,) or (N, k), k <= 16; NumPy arrays or float64 CUDA
        tensors, as solve_system takes them).  Needs no preconditioner.  On a distributed=True or shard= problem: collective,
        B and X global as for solve_system (X is read at the rows this rank owns), the norms global."""
        kind, k, _ = self._system_args("system_residuals", B, X, "X")
        L = self.L
        N = self.N
        flags = 0
        if kind == "device":
            flags = _l.SYS_DEVICE
            bk, pb, ldb = self._device_columns(B)
            xk, px, ldx = self._device_columns(X)
            self._order_torch_stream()
        else:
            bk = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(N, k))
            xk = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(N, k))
            pb, ldb, px, ldx = bk.ctypes.data, max(N, 1), xk.ctypes.data, max(N, 1)
        res, normb = np.zeros(max(k, 1)), np.zeros(max(k, 1))
        check(L.preAlps_OperatorSystemResiduals(k, pb, ldb, px, ldx, flags, _pd(res), _pd(normb)),
              "preAlps_OperatorSystemResiduals")
        return res[:k], normb[:k]

    def enable_history(self, capacity=8):
        """preAlps_SolutionHistoryCreate: keep the last `capacity` (1 .. 16) solutions of solve_system(history=True) /
        history_append on the device, in the caller's order and units; replaces an existing history.
        On a distributed=True or shard= problem the call is collective: every rank keeps the rows it owns (owned_rows) of
        every solution, m x capacity doubles (stat("hist_bytes") = 8 m capacity), and either every rank holds a ring
        afterwards or none has changed anything."""
        check(self.L.preAlps_SolutionHistoryCreate(int(capacity)), "preAlps_SolutionHistoryCreate")

    def disable_history(self):
        """preAlps_SolutionHistoryFree (close() does it too)."""
        check(self.L.preAlps_SolutionHistoryFree(), "preAlps_SolutionHistoryFree")

    def clear_history(self):
        """preAlps_SolutionHistoryClear: an empty ring of the same capacity.  On a distributed=True or shard= problem
        every rank calls it (no collective is needed: the ring's bookkeeping is the same on all of them)."""
        check(self.L.preAlps_SolutionHistoryClear(), "preAlps_SolutionHistoryClear")

    def history_project(self, B, rtol=None):
        """preAlps_SolutionHistoryProject: (x0, rank, captured) for B of shape (N,) or (N, k), k <= 16 (a NumPy array or
        a float64 CUDA tensor; x0 comes back as the same kind and shape): x0 = the element of the span of the history
        closest to the solution of A x = B in the energy norm, rank = the columns the pivoted Cholesky kept (pivots
        above rtol, default 1e-12, on the unit-diagonal Gram matrix), captured[j] = ||x0_j||_A^2.
        On a distributed=True or shard= problem the call is collective (one all-reduce): B keeps the global shape on every
        rank and is read at the rows the rank owns; x0 holds those rows and zeros in every other, so a SUM all-reduce of
        x0 over the ranks is the whole start vector (what solve_system(x0=) takes); rank and captured are global and
        have the same bits on every rank.  A NaN or Inf in a row one rank owns raises on every rank."""
        kind, k, vector = self._system_args("history_project", B, None, "x0")
        N = self.N
        flags = 0
        if kind == "device":
            import torch
            flags = _l.SYS_DEVICE
            bk, pb, ldb = self._device_columns(B)
            # several ranks: zeros in the rows this rank does not own (the library writes the owned rows and no other)
            alloc = torch.zeros if self.comm_kind != "none" else torch.empty
            x0 = alloc((k, N), dtype=torch.float64, device=bk.device).t()
            px = x0.data_ptr()
            self._order_torch_stream()
        else:
            bk = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(N, k))
            pb, ldb = bk.ctypes.data, max(N, 1)
            x0 = np.zeros((N, k), order="F")
            px = x0.ctypes.data
        rank, captured = C.c_int(), np.zeros(max(k, 1))
        check(self.L.preAlps_SolutionHistoryProject(k, pb, ldb, px, max(N, 1), flags, 0.0 if rtol is None else float(rtol),
                                                    C.byref(rank), _pd(captured)),
              "preAlps_SolutionHistoryProject")
        if vector:
            x0 = x0[:, 0].contiguous() if kind == "device" else np.ascontiguousarray(x0[:, 0])
        return x0, rank.value, captured[:k]

    def history_append(self, X):
        """preAlps_SolutionHistoryAppend: the columns of X (shape (N,) or (N, k), k <= 16; NumPy or a float64 CUDA
        tensor) enter the ring, the oldest columns leave a full one.
        On a distributed=True or shard= problem the call is collective (two all-reduces and one halo exchange): X keeps
        the global shape and is read at the rows this rank owns alone, so the x of solve_system can be appended as it
        came back, without assembling it.  A NaN or Inf in a row one rank owns raises on every rank, and the history
        is then unchanged on all of them."""
        kind, k, _ = self._system_args("history_append", X, None, "x0")
        N = self.N
        if kind == "device":
            xk, px, ldx = self._device_columns(X)
            self._order_torch_stream()
        else:
            xk = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(N, k))
            px, ldx = xk.ctypes.data, max(N, 1)
        check(self.L.preAlps_SolutionHistoryAppend(k, px, ldx, _l.SYS_DEVICE if kind == "device" else 0),
              "preAlps_SolutionHistoryAppend")

    def reference_rhs(self):
        rhs = np.zeros(self.m)
        check(self.L.preAlps_hip_reference_rhs(_pd(rhs)), "preAlps_hip_reference_rhs")
        return rhs

    def local_csr(self):
        """Host copy of the local row panel (global column ids)."""
        m, nnz = self.A.info.m, self.A.info.lnnz
        rp = np.ctypeslib.as_array(self.A.rowPtr, shape=(m + 1,)).copy()
        ci = np.ctypeslib.as_array(self.A.colInd, shape=(max(nnz, 1),))[:nnz].copy()
        v = np.ctypeslib.as_array(self.A.val, shape=(max(nnz, 1),))[:nnz].copy()
        return rp, ci, v

    def stat(self, key):
        v = C.c_double()
        if self.L.preAlps_hip_get_stat(key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return v.value

    def new_ecg(self, t, ortho_alg=ORTHODIR, bs_red=NO_BS_RED, tol=1e-5, max_iter=1000):
        e = preAlps_ECG_t()
        e.comm = 0x44000000
        e.globPbSize, e.locPbSize = self.M, self.m
        e.maxIter, e.enlFac, e.tol = max_iter, t, tol
        e.ortho_alg, e.bs_red = ortho_alg, bs_red
        return e

    def solve(self, rhs, t, ortho_alg=ORTHODIR, bs_red=NO_BS_RED, tol=1e-5, max_iter=1000, x0=None):
        """preAlps_ECGSolve = the reference driver loop, in C.  x0 (m values): start the iteration from it
        (preAlps_ECGSolveGuess with one system) instead of from zero; the result then carries sys_res0, the norm of
        the split of b - A x0, and iters = 0 with x = x0 if that already meets tol * ||b||."""
        if x0 is not None:
            xs = np.shape(x0)
            if len(xs) != 1:
                raise ValueError("x0 must be one-dimensional (m values), not of shape %r" % (xs,))
            if xs[0] != self.m:
                raise ValueError("x0 has %d rows, the operator has %d local rows" % (xs[0], self.m))
            bshape = np.shape(rhs)
            if len(bshape) != 1 or bshape[0] != self.m:
                raise ValueError("rhs must hold the %d local rows, not be of shape %r" % (self.m, bshape))
            got = self.solve_multi(np.asarray(rhs, dtype=np.float64)[:, None], t, ortho_alg, bs_red, tol, max_iter,
                                   X0=np.asarray(x0, dtype=np.float64)[:, None])
            got.x = np.ascontiguousarray(got.x[:, 0])
            return got
        if not self.has_precond:
            self.create_block_jacobi()
        import time
        L = self.L
        check(L.preAlps_hip_prepare_operator(int(t)), "preAlps_hip_prepare_operator")
        e = self.new_ecg(t, ortho_alg, bs_red, tol, max_iter)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        sol = np.zeros(self.m)
        cap = max_iter + 2
        res = np.zeros(cap)
        bs = np.zeros(cap, dtype=np.int32)
        nh = C.c_int()
        t0 = time.perf_counter()
        check(L.preAlps_ECGSolve(C.byref(e), _pd(rhs), _pd(sol), _pd(res), _pi(bs), cap, C.byref(nh)),
              "preAlps_ECGSolve")
        dt = time.perf_counter() - t0
        timers = {k: getattr(e, k) for k in ("tot_t", "comm_t", "trsm_t", "gemm_t", "potrf_t", "copy_t")}
        return EcgResult(x=sol, iters=e.iter, res=res[:nh.value].copy(), bs=bs[:nh.value].copy(),
                         final_res=e.res, final_bs=e.bs, normb=e.normb, seconds=dt, timers=timers)

    def solve_multi(self, B, t, ortho_alg=ORTHODIR, bs_red=NO_BS_RED, tol=1e-5, max_iter=1000, X0=None):
        """preAlps_ECGSolveMulti: the k columns of B (m x k) as k systems solved by one block iteration of
        enlarging factor t, a multiple of k; system j owns the columns j*t/k .. (j+1)*t/k - 1 of the panels.
        Returns an EcgResult with x of shape (m, k), res / bs as solve() (the Frobenius norm of all of R) and
        sys_res, sys_normb (k values) and sys_hist (iterations x k): the per-system residual norms the
        stopping test uses.  ||b_j - A x_j|| <= sqrt(t / k) * sys_res[j] in exact arithmetic.
        X0 (m x k): a starting value for every system (preAlps_ECGSolveGuess); sys_res0 then holds the k residual
        norms the iteration starts from, and a guess that already meets every threshold comes back as x after no
        iteration.  X0 = None is preAlps_ECGSolveMulti as before.
        On a distributed problem B, X0 and x hold this rank's m rows; sys_normb, sys_hist, sys_res0, res and normb are
        global and equal on all ranks.  What the library refuses (PreAlpsError) is raised on every rank.  The shape
        checks of this method (ValueError) are made before the library is entered and are this rank's alone: a rank
        that fails them never joins the collective start, so the caller must pass well-shaped arrays on every rank
        (each rank can test its own against prob.m beforehand)."""
        Bs = np.shape(B)
        if len(Bs) != 2:
            raise ValueError("B must be two-dimensional (m x k), not of shape %r" % (Bs,))
        if Bs[0] != self.m:
            raise ValueError("B has %d rows, the operator has %d local rows" % (Bs[0], self.m))
        k = int(Bs[1])
        if k < 1 or int(t) % k != 0:
            raise ValueError("the enlarging factor t = %d is not a multiple of the %d right-hand sides" % (t, k))
        if X0 is not None:
            Xs = np.shape(X0)
            if len(Xs) != 2:
                raise ValueError("X0 must be two-dimensional (m x k), not of shape %r" % (Xs,))
            if Xs[0] != self.m:
                raise ValueError("X0 has %d rows, the operator has %d local rows" % (Xs[0], self.m))
            if Xs[1] != k:
                raise ValueError("X0 has %d columns, B has %d right-hand sides" % (Xs[1], k))
        if not self.has_precond:
            self.create_block_jacobi()
        import time
        L = self.L
        check(L.preAlps_hip_prepare_operator(int(t)), "preAlps_hip_prepare_operator")
        e = self.new_ecg(t, ortho_alg, bs_red, tol, max_iter)
        B = np.asfortranarray(B, dtype=np.float64)
        ld = max(self.m, 1)
        sol = np.zeros((self.m, k), order="F")
        cap = max_iter + 2
        res = np.zeros(cap)
        bs = np.zeros(cap, dtype=np.int32)
        sys_hist = np.zeros((cap, k), order="F")
        sys_normb = np.zeros(k)
        sys_res = np.zeros(k)
        nh = C.c_int()
        sys_res0 = None
        if X0 is not None:
            X0 = np.asfortranarray(X0, dtype=np.float64)
            sys_res0 = np.zeros(k)
        t0 = time.perf_counter()
        if X0 is None:
            check(L.preAlps_ECGSolveMulti(C.byref(e), k, _pd(B), ld, _pd(sol), ld, _pd(res), _pi(bs), _pd(sys_hist),
                                          _pd(sys_normb), cap, C.byref(nh)), "preAlps_ECGSolveMulti")
        else:
            check(L.preAlps_ECGSolveGuess(C.byref(e), k, _pd(B), ld, _pd(X0), ld, _pd(sol), ld, _pd(res), _pi(bs),
                                          _pd(sys_hist), _pd(sys_normb), _pd(sys_res0), cap, C.byref(nh)),
                  "preAlps_ECGSolveGuess")
        dt = time.perf_counter() - t0
        n = nh.value
        if n:
            sys_res = sys_hist[n - 1].copy()
        elif sys_res0 is not None:
            sys_res = sys_res0.copy()
        timers = {k_: getattr(e, k_) for k_ in ("tot_t", "comm_t", "trsm_t", "gemm_t", "potrf_t", "copy_t")}
        return EcgResult(x=sol, iters=e.iter, res=res[:n].copy(), bs=bs[:n].copy(), final_res=e.res,
                         final_bs=e.bs, normb=e.normb, seconds=dt, timers=timers, sys_res=sys_res,
                         sys_normb=sys_normb, sys_hist=np.ascontiguousarray(sys_hist[:n]), sys_res0=sys_res0)

    # -- single operations, for tests and micro-benchmarks -----------------------
    def panel(self, ncols, t):
        """Allocate an m x ncols device panel laid out for enlarging factor t."""
        d = CPLM_Mat_Dense_t()
        check(self.L.preAlps_hip_panel_alloc(C.byref(d), self.M, ncols, self.m, ncols, t),
              "preAlps_hip_panel_alloc")
        return d

    def panel_free(self, d):
        self.L.preAlps_hip_panel_free(C.byref(d))

    def to_device(self, d, host, t):
        host = np.asfortranarray(host, dtype=np.float64)
        check(self.L.preAlps_hip_panel_from_host(C.byref(d), t, _pd(host), host.shape[0]),
              "preAlps_hip_panel_from_host")

    def to_host(self, d, t):
        out = np.zeros((d.info.m, d.info.n), order="F")
        check(self.L.preAlps_hip_panel_to_host(C.byref(d), t, _pd(out), max(d.info.m, 1)),
              "preAlps_hip_panel_to_host")
        return out

    def block_operator(self, X, t):
        """AX = A X for a host (m x n) array; goes through preAlps_BlockOperator."""
        n = X.shape[1]
        dx, dy = self.panel(n, t), self.panel(n, t)
        try:
            self.to_device(dx, X, t)
            check(self.L.preAlps_BlockOperator(C.byref(dx), C.byref(dy)), "preAlps_BlockOperator")
            return self.to_host(dy, t)
        finally:
            self.panel_free(dx)
            self.panel_free(dy)

    def block_jacobi_apply(self, X, t):
        if not self.has_precond:
            self.create_block_jacobi()
        n = X.shape[1]
        dx, dy = self.panel(n, t), self.panel(n, t)
        try:
            self.to_device(dx, X, t)
            check(self.L.preAlps_BlockJacobiApply(C.byref(dx), C.byref(dy)), "preAlps_BlockJacobiApply")
            return self.to_host(dy, t)
        finally:
            self.panel_free(dx)
            self.panel_free(dy)

    def sync(self):
        check(self.L.preAlps_hip_sync(), "preAlps_hip_sync")

    def close(self):
        self.L.preAlps_BlockJacobiFree()
        self.L.preAlps_OperatorFree()
        if getattr(self, "_set_precision", False):      # (the library's setting: back to the default if this problem moved it)
            self.L.preAlps_hip_set_operator_precision(0)
            self._set_precision = False
        self.has_precond = False
        if getattr(self, "_plan_only", False):
            self.L.preAlps_hip_plan_only(0)
            self._plan_only = False
