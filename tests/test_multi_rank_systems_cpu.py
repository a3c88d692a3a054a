"""Several right-hand sides and a start from a guess on more than one rank: what can be checked without a GPU, with the
mechanism of test_distributed_cpu.py -- gloo ranks that plan their shard with the C library in plan-only mode.

1. A refusal that depends on one rank's arguments is agreed on before any rank returns: rank 1 passes ldrhs = m - 1,
   and BOTH ranks come back refused -- rank 1 with its reason, rank 0 with "another process of the group refused" --
   instead of one of them waiting in a collective.  (The all-reduce hook of the test sums one host word with gloo: in
   plan-only mode there is no device, and the word the ranks agree on is host memory.)
2. The column every local row starts in, p % s with p the GLOBAL part index (preAlps_hip_system_columns, the array the
   start uploads), is on each rank the slice [lo, hi) of the one-process array."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(L, n, nparts, rank, world):
    from prealps_amd import gen
    from prealps_amd.lib import check
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    check(L.preAlps_hip_set_world(rank, world), "set_world")
    rp, ci, v = gen.poisson3d_csr(n)
    check(L.preAlps_OperatorBuildFromCSR(n ** 3, rp.ctypes.data_as(pi), ci.ctypes.data_as(pi), v.ctypes.data_as(pd),
                                         nparts, None, 1), "build")
    M, m = C.c_int(), C.c_int()
    check(L.preAlps_OperatorGetSizes(C.byref(M), C.byref(m)), "sizes")
    rpp, nrp = pi(), C.c_int()
    check(L.preAlps_OperatorGetRowPosPtr(C.byref(rpp), C.byref(nrp)), "rowpos")
    rowpos = np.ctypeslib.as_array(rpp, shape=(nrp.value,)).copy()
    return M.value, m.value, rowpos


def _worker(rank, world, port, what, q):
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
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        n, nparts = 8, 8
        out = None
        if what == "pcol":
            # the one-process array first (the same deterministic build on every rank), then this rank's shard
            M, m1, rowpos = _build(L, n, nparts, 0, 1)
            assert m1 == M == n ** 3
            whole = {}
            for s in (1, 2):
                whole[s] = np.full(M, -1, dtype=np.int32)
                check(L.preAlps_hip_system_columns(s, whole[s].ctypes.data_as(pi)), "system_columns")
                want = np.repeat(np.arange(nparts) % s, np.diff(rowpos)).astype(np.int32)
                np.testing.assert_array_equal(whole[s], want)
            L.preAlps_OperatorFree()
            M, m, rowpos2 = _build(L, n, nparts, rank, world)
            np.testing.assert_array_equal(rowpos2, rowpos)
            p0, p1 = rank * nparts // world, (rank + 1) * nparts // world
            lo, hi = int(rowpos[p0]), int(rowpos[p1])
            assert m == hi - lo
            for s in (1, 2):
                mine = np.full(m, -1, dtype=np.int32)
                check(L.preAlps_hip_system_columns(s, mine.ctypes.data_as(pi)), "system_columns")
                np.testing.assert_array_equal(mine, whole[s][lo:hi])
            out = (lo, hi)
        else:
            M, m, rowpos = _build(L, n, nparts, rank, world)

            def allreduce(ctx, ptr, count):          # plan-only: the word is host memory
                a = np.ctypeslib.as_array(C.cast(ptr, pd), shape=(count,))
                t = torch.from_numpy(a.copy())
                dist.all_reduce(t)
                a[:] = t.numpy()
                return 0

            ar = pl.ALLREDUCE_FN(allreduce)
            check(L.preAlps_hip_set_comm(ar, pl.EXCHANGE_FN(), None), "set_comm")
            e = pa.preAlps_ECG_t()
            e.comm = 0x44000000
            e.globPbSize, e.locPbSize = M, m
            e.maxIter, e.enlFac, e.tol = 100, 4, 1e-5
            e.ortho_alg, e.bs_red = pa.ORTHODIR, pa.NO_BS_RED
            B = np.asfortranarray(np.random.default_rng(7).standard_normal((m, 2)))
            rci = C.c_int(0)
            ld = m - 1 if rank == 1 else m
            rc = L.preAlps_ECGInitializeMulti(C.byref(e), 2, B.ctypes.data_as(pd), ld, C.byref(rci))
            out = (rc, L.preAlps_hip_last_error().decode(), m)
            check(L.preAlps_hip_set_comm(pl.ALLREDUCE_FN(), pl.EXCHANGE_FN(), None), "set_comm")
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", out))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc()), None))


def _run(world, what):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, what, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] == "ok", r
    return {r[0]: r[2] for r in res}


def test_the_riding_sums_need_a_buffer():
    """pa_k_group_norms_ride refuses a missing buffer on the host, before any HIP call (no launch, no GPU)."""
    import prealps_amd
    L = prealps_amd.load()
    L.pa_rt_error.restype = C.c_char_p
    assert L.pa_k_group_norms_ride(None, 0, 4, 2, 2, None, None) == 1
    assert "pa_k_group_norms_ride: no buffer for the 2 sums" in L.pa_rt_error().decode()
    assert L.pa_k_group_norms_ride(None, 0, 4, 3, 2, None, None) == 1
    assert "3 systems of 2 columns do not fit a panel of stride 4" in L.pa_rt_error().decode()


def test_a_refusal_of_one_rank_is_returned_by_both():
    got = _run(2, "agree")
    (rc0, msg0, m0), (rc1, msg1, m1) = got[0], got[1]
    assert rc0 != 0 and rc1 != 0, got
    for msg in (msg0, msg1):
        assert "preAlps_ECGInitializeMulti" in msg and "single process" not in msg, msg
    assert "ldrhs = %d is smaller than the %d local rows" % (m1 - 1, m1) in msg1, msg1
    assert "another process of the group refused" in msg0, msg0


@pytest.mark.parametrize("world", [2, 3])
def test_the_column_of_every_row_is_a_slice_of_the_one_process_array(world):
    got = _run(world, "pcol")
    spans = [got[r] for r in range(world)]
    assert spans[0][0] == 0 and spans[-1][1] == 8 ** 3
    assert all(spans[r][1] == spans[r + 1][0] for r in range(world - 1))
