"""The caller's own system (preAlps_ECGSolveSystem) on more than one rank: what can be checked without a GPU, with the
mechanism of test_multi_rank_systems_cpu.py -- two gloo ranks that plan their shard of Poisson 8^3 in 8 parts with the C
library in plan-only mode (the word the ranks agree on is host memory, summed with gloo).

(a) With good arguments the start is no longer refused for the number of processes: both ranks agree on the arguments
    and are then refused for the one reason left, "plan-only mode".
(b) A leading dimension is one rank's argument: rank 1 passes ldb = N - 1 and BOTH ranks come back refused -- rank 1
    with its reason, rank 0 with "another process of the group refused" -- and none waits in a collective.
(c) preAlps_OperatorGetOwnedRows is on each rank the slice [lo, hi) of the one-process permutation; the slices
    partition 0 .. N-1.

One spawn of the two ranks serves the three tests."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SIDE, NPARTS, WORLD = 8, 8, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(L, rank, world):
    from prealps_amd import gen
    from prealps_amd.lib import check
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    check(L.preAlps_hip_set_world(rank, world), "set_world")
    rp, ci, v = gen.poisson3d_csr(N_SIDE)
    check(L.preAlps_OperatorBuildFromCSR(N_SIDE ** 3, rp.ctypes.data_as(pi), ci.ctypes.data_as(pi), v.ctypes.data_as(pd),
                                         NPARTS, None, 1), "build")
    M, m = C.c_int(), C.c_int()
    check(L.preAlps_OperatorGetSizes(C.byref(M), C.byref(m)), "sizes")
    rpp, nrp = pi(), C.c_int()
    check(L.preAlps_OperatorGetRowPosPtr(C.byref(rpp), C.byref(nrp)), "rowpos")
    rowpos = np.ctypeslib.as_array(rpp, shape=(nrp.value,)).copy()
    pp, pn = pi(), C.c_int()
    check(L.preAlps_OperatorGetPermPtr(C.byref(pp), C.byref(pn)), "perm")
    perm = np.ctypeslib.as_array(pp, shape=(pn.value,)).copy()
    return M.value, m.value, rowpos, perm


def _owned(L):
    from prealps_amd.lib import check
    rows, m = C.POINTER(C.c_int)(), C.c_int(-1)
    check(L.preAlps_OperatorGetOwnedRows(C.byref(rows), C.byref(m)), "owned rows")
    return np.ctypeslib.as_array(rows, shape=(m.value,)).copy()


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        import torch
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import prealps_amd as pa
        import prealps_amd.lib as pl
        from prealps_amd.lib import check
        L = pa.load()
        L.preAlps_hip_plan_only(1)
        pd = C.POINTER(C.c_double)
        out = {}
        # (c) the one-process permutation first (the same deterministic build on every rank), then this rank's shard
        M, m1, rowpos, perm1 = _build(L, 0, 1)
        assert m1 == M == N_SIDE ** 3
        np.testing.assert_array_equal(_owned(L), perm1)
        L.preAlps_OperatorFree()
        M, m, rowpos2, perm = _build(L, rank, world)
        np.testing.assert_array_equal(rowpos2, rowpos)
        np.testing.assert_array_equal(perm, perm1)
        p0, p1 = rank * NPARTS // world, (rank + 1) * NPARTS // world
        lo, hi = int(rowpos[p0]), int(rowpos[p1])
        mine = _owned(L)
        assert m == hi - lo == len(mine)
        np.testing.assert_array_equal(mine, perm1[lo:hi])
        out["rows"] = (lo, hi, mine)

        def allreduce(ctx, ptr, count):          # plan-only: the word is host memory
            a = np.ctypeslib.as_array(C.cast(ptr, pd), shape=(count,))
            t = torch.from_numpy(a.copy())
            dist.all_reduce(t)
            a[:] = t.numpy()
            return 0

        ar = pl.ALLREDUCE_FN(allreduce)
        check(L.preAlps_hip_set_comm(ar, pl.EXCHANGE_FN(), None), "set_comm")
        B = np.asfortranarray(np.random.default_rng(7).standard_normal((M, 2)))
        x = np.zeros((M, 2), order="F")
        nh = C.c_int(0)

        def solve(ldb):
            e = pa.preAlps_ECG_t()
            e.comm = 0x44000000
            e.globPbSize, e.locPbSize = M, m
            e.maxIter, e.enlFac, e.tol = 100, 4, 1e-5
            e.ortho_alg, e.bs_red = pa.ORTHODIR, pa.NO_BS_RED
            rc = L.preAlps_ECGSolveSystem(C.byref(e), 2, B.ctypes.data, ldb, None, 0, x.ctypes.data, M,
                                          pl.SYS_STOP_ORIGINAL, None, None, None, None, None, 0, C.byref(nh))
            return rc, L.preAlps_hip_last_error().decode()

        out["good"] = solve(M)                                   # (a)
        out["ldb"] = solve(M - 1 if rank == 1 else M)            # (b)
        out["N"] = M
        assert not x.any()                                       # a refused solve writes nothing
        check(L.preAlps_hip_set_comm(pl.ALLREDUCE_FN(), pl.EXCHANGE_FN(), None), "set_comm")
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", out))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc()), None))


@pytest.fixture(scope="module")
def ranks():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=180) for _ in procs]        # (a rank that waits in a collective shows here, not as a hang)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in res:
        assert r[1] == "ok", r
    return {r[0]: r[2] for r in res}


def test_good_arguments_are_refused_for_plan_only_mode_alone(ranks):
    for r in range(WORLD):
        rc, msg = ranks[r]["good"]
        assert rc != 0, ranks
        assert "preAlps_ECGSolveSystem" in msg and "plan-only mode" in msg, msg
        assert "single process" not in msg, msg


def test_a_short_ldb_on_one_rank_is_refused_by_both(ranks):
    (rc0, msg0), (rc1, msg1) = ranks[0]["ldb"], ranks[1]["ldb"]
    N = ranks[1]["N"]
    assert rc0 != 0 and rc1 != 0, ranks
    for msg in (msg0, msg1):
        assert "preAlps_ECGSolveSystem" in msg and "single process" not in msg, msg
    assert "ldb = %d is smaller than the %d rows of the matrix" % (N - 1, N) in msg1, msg1
    assert "another process of the group refused" in msg0, msg0


def test_owned_rows_are_slices_of_the_permutation_and_partition_the_rows(ranks):
    spans = [ranks[r]["rows"] for r in range(WORLD)]
    N = ranks[0]["N"]
    assert spans[0][0] == 0 and spans[-1][1] == N
    assert all(spans[r][1] == spans[r + 1][0] for r in range(WORLD - 1))
    every = np.concatenate([s[2] for s in spans])
    np.testing.assert_array_equal(np.sort(every), np.arange(N))


def test_the_riding_launcher_refuses_on_the_host():
    """pa_k_sys_norms_ride refuses k * s > ts and a missing buffer before any HIP call (no launch, no GPU)."""
    import prealps_amd
    L = prealps_amd.load()
    L.pa_rt_error.restype = C.c_char_p
    assert L.pa_k_sys_norms_ride(None, 0, None, 0, 4, 3, 2, None, None) == 1
    assert "3 systems of 2 columns do not fit a panel of stride 4" in L.pa_rt_error().decode()
    assert L.pa_k_sys_norms_ride(None, 0, None, 0, 4, 2, 2, None, None) == 1
    assert "pa_k_sys_norms_ride: no buffer for the 2 sums" in L.pa_rt_error().decode()
