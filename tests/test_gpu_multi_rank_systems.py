"""Several right-hand sides and a start from an initial guess on more than one rank (preAlps_ECGSolveMulti /
preAlps_ECGSolveGuess through EcgProblem.solve_multi on a distributed problem): ranks that share the one GPU of the
test box and talk through gloo, shaped like test_gpu_distributed.py.  Every rank passes and receives its own rows.

The expected values come from the CPU oracle (oracle.ECG: the restated reference iteration) started from
R0 = [b_1 | ... | b_k] instead of the split of one right-hand side: _oracle_multi below drives the oracle's own
reverse-communication entry points, writes that start into its R panel, and applies the per-system stopping test.
The problem is Poisson 16^3 in boxes of (4, 4, 8) with t = 4; the right-hand sides are seeded standard-normal columns
on the global rows, each rank taking its rows [lo, hi).  Tolerances against the oracle are those of
test_gpu_distributed.py::test_two_ranks_one_gpu_match_oracle.

One spawn per process group; a worker makes one build and runs its cases on it:
  world 2: (1) k = 4, s = 1, Orthodir; (2) k = 2, s = 2, Orthomin; (4) a guess -- the library's own 1e-3 solution
           (fewer iterations, start residuals against scipy), X0 = 0 (bitwise the cold solve), a guess that already
           meets every threshold (no iteration, x = x0); (5) refusals reached together -- a NaN in rank 0's x0, a
           right-hand side that is zero on rank 1's rows only (NOT refused), one that is zero everywhere; (6) an
           iteration of four systems costs as many all-reduces as an iteration of one.  Beside those: the stopping
           test that reduces the norm by itself (PREALPS_ECG_LAZY_STOP=0), and the caller's own loop over the RCI
           entries -- the two other places where the per-system sums ride on a collective.
  world 4: (3) k = 4, s = 1: every rank has more than one neighbour, the histories are identical on all ranks.
  one process: (7) a preAlps_hip_loopback shard runs solve_multi."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
N1, BOX, T = 16, (4, 4, 8), 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_multi(O, Bm, rowpos, G, s, alg, tol=TOL, max_iter=1000):
    """The oracle's iteration from R0 = [b_1 | ... | b_k]: system j in the columns j*s .. j*s + s - 1, a row of part p
    puts b_j into column j*s + p % s.  The loop is the reference driver's (orc_ecg_solve), with the oracle's own
    preconditioner and product; the stopping test is per system, g_j against tol * ||b_j||."""
    N, k = G.shape
    t = k * s
    ref = O.ECG(Bm, rowpos, t, alg, O.NO_BS_RED, tol, max_iter)
    L, e = ref.L, ref.e
    rci, stop = C.c_int(0), C.c_int(0)
    assert L.orc_ecg_initialize(e, np.zeros(N), C.byref(rci)) == 0
    R = ref.panel(2, t)
    R[:] = 0.0
    for p in range(len(rowpos) - 1):
        for j in range(k):
            R[rowpos[p]:rowpos[p + 1], j * s + p % s] = G[rowpos[p]:rowpos[p + 1], j]
    nb = np.linalg.norm(G, axis=0)
    rp, ci, v = ref.csr

    def ptr(which):
        return L.orc_ecg_panel(e, which)

    L.orc_bj_apply(ref.bj.h, t, ptr(2), N, ptr(0), N)
    L.orc_spmm(N, rp, ci, v, t, ptr(0), N, ptr(1), N)
    res, hist = [], []
    while True:
        assert L.orc_ecg_iterate(e, C.byref(rci)) == 0
        if rci.value == 0:
            L.orc_spmm(N, rp, ci, v, t, ptr(0), N, ptr(1), N)
            continue
        L.orc_ecg_stopping(e, C.byref(stop))          # (for the Frobenius norm; its decision is the one-system test)
        g = np.sqrt((np.asarray(ref.panel(2, t)) ** 2).reshape(N, k, s).sum(axis=(0, 2)))
        res.append(L.orc_ecg_res(e))
        hist.append(g)
        if not (g > tol * nb).any() or L.orc_ecg_iter(e) >= max_iter:
            break
        L.orc_bj_apply(ref.bj.h, t, ptr(2) if alg == O.ORTHOMIN else ptr(1), N, ptr(3), N)
    x = np.asarray(ref.panel(4, t)).reshape(N, k, s).sum(axis=2)
    return dict(iters=L.orc_ecg_iter(e), res=np.array(res), hist=np.array(hist), x=x, nb=nb)


def _against_oracle(got, ref, lo, hi):
    assert got.iters == ref["iters"], (got.iters, ref["iters"])
    np.testing.assert_allclose(got.res, ref["res"], rtol=1e-8)
    np.testing.assert_allclose(got.sys_hist[-1], ref["hist"][-1], rtol=1e-6)
    np.testing.assert_allclose(got.x, ref["x"][lo:hi], rtol=1e-7, atol=1e-9 * np.abs(ref["x"]).max())
    np.testing.assert_allclose(got.sys_normb, ref["nb"], rtol=1e-13)
    assert (got.sys_res <= TOL * got.sys_normb).all()


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["LOCAL_RANK"] = "0"
        if world == 4:
            os.environ["PREALPS_HALO_OVERLAP"] = "1"
        import torch  # noqa: F401
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import prealps_amd as pa
        from prealps_amd import gen
        from oracle import oracle as O
        import scipy.sparse as sp
        rp, ci, v = gen.poisson3d_csr(N1)
        part, nparts = gen.box_partition(N1, BOX)
        prob = pa.EcgProblem(rp, ci, v, nparts, part, scale=True, device=0, distributed=True)
        A = sp.csr_matrix((v, ci, rp), shape=(N1 ** 3, N1 ** 3))
        Bm, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, nparts)
        bounds = [int(rowpos[r * nparts // world]) for r in range(world + 1)]
        lo, hi = bounds[rank], bounds[rank + 1]
        assert prob.m == hi - lo and prob.stat("halo_rows") > 0
        G = np.random.default_rng(20261019).standard_normal((N1 ** 3, 4))
        fails = []

        def gathered(obj):
            box = [None] * world
            dist.all_gather_object(box, obj)
            return box

        def case(name, fn):
            try:
                fn()
            except Exception as e:
                import traceback
                fails.append("case %s: %s\n%s" % (name, e, traceback.format_exc()))

        cold = {}

        # (1) / (3): k = 4, s = 1, Orthodir
        def four_systems():
            got = cold["odir"] = prob.solve_multi(G[lo:hi], T, tol=TOL)
            nbs = gathered(got.sys_normb.tobytes())
            hists = gathered(got.sys_hist.tobytes())
            ress = gathered(got.res.tobytes())
            ref = _oracle_multi(O, Bm, rowpos, G, 1, O.ORTHODIR)
            print("rank", rank, "k=4 s=1 odir iters", got.iters, ref["iters"], "res", got.res[-1], ref["res"][-1],
                  "sys", got.sys_hist[-1] / ref["hist"][-1] - 1.0, flush=True)
            _against_oracle(got, ref, lo, hi)
            assert got.x.shape == (hi - lo, 4) and got.sys_hist.shape == (got.iters, 4)
            assert all(b == nbs[0] for b in nbs), "sys_normb differs between the ranks"
            assert all(h == hists[0] for h in hists), "sys_hist differs between the ranks"
            assert all(r == ress[0] for r in ress), "res differs between the ranks"
            assert got.normb == pytest.approx(np.linalg.norm(G), rel=1e-13)

        case("four systems", four_systems)

        if world == 2:
            # (2): two columns per system cross the part-to-column rule, Orthomin
            def two_by_two():
                got = prob.solve_multi(G[lo:hi, :2], T, ortho_alg=pa.ORTHOMIN, tol=TOL)
                nbs = gathered(got.sys_normb.tobytes())
                ref = _oracle_multi(O, Bm, rowpos, G[:, :2], 2, O.ORTHOMIN)
                print("rank", rank, "k=2 s=2 omin iters", got.iters, ref["iters"], "res", got.res[-1], ref["res"][-1],
                      "sys", got.sys_hist[-1] / ref["hist"][-1] - 1.0, flush=True)
                _against_oracle(got, ref, lo, hi)
                assert all(b == nbs[0] for b in nbs), "sys_normb differs between the ranks"

            case("two by two", two_by_two)

            # (4): a start from a guess
            def guess():
                first = cold["odir"]
                x0 = prob.solve_multi(G[lo:hi], T, tol=1e-3).x
                warm = prob.solve_multi(G[lo:hi], T, tol=TOL, X0=x0)
                x0g = np.vstack(gathered(x0))
                zero = prob.solve_multi(G[lo:hi], T, tol=TOL, X0=np.zeros((hi - lo, 4)))
                tight = prob.solve_multi(G[lo:hi], T, tol=1e-8).x
                done = prob.solve_multi(G[lo:hi], T, tol=TOL, X0=tight)
                r0 = np.linalg.norm(G - Bm @ x0g, axis=0)
                print("rank", rank, "guess iters", warm.iters, "cold", first.iters, "sys_res0 / scipy - 1",
                      warm.sys_res0 / r0 - 1.0, flush=True)
                assert 0 < warm.iters < first.iters, (warm.iters, first.iters)
                assert (warm.sys_res <= TOL * warm.sys_normb).all()
                np.testing.assert_allclose(warm.sys_res0, r0, rtol=1e-10)
                assert warm.sys_normb.tobytes() == first.sys_normb.tobytes()
                assert zero.iters == first.iters
                assert zero.res.tobytes() == first.res.tobytes() and zero.bs.tobytes() == first.bs.tobytes()
                assert zero.x.tobytes() == first.x.tobytes()
                assert done.iters == 0 and len(done.res) == 0
                assert np.array_equal(done.x, tight)

            case("guess", guess)

            # ... and solve(b, t, x0=): ONE system from a guess, whose ||b||^2 is the host sum of preAlps_ECGSolve
            # reduced over the ranks (normb bitwise that of solve(b, t)) and whose stopping test is the scalar one
            def one_system_guess():
                b = prob.reference_rhs()
                first = prob.solve(b, T, tol=TOL)
                x0 = prob.solve(b, T, tol=1e-3).x
                warm = prob.solve(b, T, tol=TOL, x0=x0)
                x0g, xg = np.concatenate(gathered(x0)), np.concatenate(gathered(warm.x))
                nbs = gathered((warm.normb, warm.sys_res0.tobytes(), warm.res.tobytes()))
                bg = O.reference_rhs(rowpos)
                # (every row lies in exactly one column of the split, so its Frobenius norm is ||b - A x0||_2)
                r0, true = np.linalg.norm(bg - Bm @ x0g), np.linalg.norm(bg - Bm @ xg)
                print("rank", rank, "one system: iters", warm.iters, "cold", first.iters, "sys_res0 / scipy - 1",
                      warm.sys_res0[0] / r0 - 1.0, "true / res", true / warm.final_res, flush=True)
                assert warm.x.shape == (hi - lo,) and warm.normb == first.normb and warm.sys_normb[0] == first.normb
                np.testing.assert_allclose(warm.sys_res0, [r0], rtol=1e-10)
                assert 0 < warm.iters < first.iters, (warm.iters, first.iters)
                assert warm.final_res <= TOL * warm.normb
                # true against recurrence residual: the factor 4.0 and the 1e-12 of test_gpu_multi_rhs.py, s = 4
                assert true <= 4.0 * np.sqrt(T) * warm.final_res + 1e-12, (true, warm.final_res)
                assert all(n == nbs[0] for n in nbs), "normb, sys_res0 or res differ between the ranks"

            case("one system from a guess", one_system_guess)

            # (5): refusals that both ranks reach
            def refusals():
                x0 = np.zeros((hi - lo, 4))
                if rank == 0:
                    x0[(hi - lo) // 2, 1] = np.nan
                with pytest.raises(pa.PreAlpsError, match="preAlps_ECGInitializeGuess.*not finite"):
                    prob.solve_multi(G[lo:hi], T, tol=TOL, X0=x0)
                Gz = G.copy()
                Gz[bounds[1]:bounds[2], 2] = 0.0          # zero on rank 1's rows only: its global norm is not zero
                got = prob.solve_multi(Gz[lo:hi], T, tol=TOL)
                ref = _oracle_multi(O, Bm, rowpos, Gz, 1, O.ORTHODIR)
                print("rank", rank, "locally zero rhs iters", got.iters, ref["iters"], flush=True)
                assert got.iters == ref["iters"], (got.iters, ref["iters"])
                np.testing.assert_allclose(got.sys_normb, ref["nb"], rtol=1e-13)
                Gz[:, 2] = 0.0
                with pytest.raises(pa.PreAlpsError, match="preAlps_ECGInitializeMulti.*right-hand side 2 has norm zero"):
                    prob.solve_multi(Gz[lo:hi], T, tol=TOL)
                # ... and the ranks are together afterwards
                again = prob.solve_multi(G[lo:hi], T, tol=TOL)
                assert again.res.tobytes() == cold["odir"].res.tobytes()

            case("refusals", refusals)

            # beside the issue's cases: PREALPS_ECG_LAZY_STOP=0 (read at every start) reduces the norm by itself, before
            # the decision -- there the k sums ride behind the pair [norm^2, status] in that all-reduce
            def eager():
                os.environ["PREALPS_ECG_LAZY_STOP"] = "0"
                try:
                    got = prob.solve_multi(G[lo:hi], T, tol=TOL)
                finally:
                    del os.environ["PREALPS_ECG_LAZY_STOP"]
                hists = gathered(got.sys_hist.tobytes())
                ref = _oracle_multi(O, Bm, rowpos, G, 1, O.ORTHODIR)
                print("rank", rank, "eager stopping test iters", got.iters, ref["iters"], "sys",
                      got.sys_hist[-1] / ref["hist"][-1] - 1.0, flush=True)
                _against_oracle(got, ref, lo, hi)
                assert all(h == hists[0] for h in hists), "sys_hist differs between the ranks"
                np.testing.assert_allclose((got.sys_hist ** 2).sum(axis=1), got.res ** 2, rtol=1e-12)

            case("eager", eager)

            # ... and the caller's own loop over the RCI entries (the loop of test_gpu_multi_rhs.py): there
            # preAlps_ECGStoppingCriterion reduces the norm, and with it the k sums the update left behind
            def callers_loop():
                from prealps_amd.lib import check
                L, k, m = prob.L, 2, hi - lo
                Bl = np.asfortranarray(G[lo:hi, :k])
                want = prob.solve_multi(Bl, T, tol=TOL)
                pd = C.POINTER(C.c_double)
                e = prob.new_ecg(T, pa.ORTHODIR, pa.NO_BS_RED, TOL, 1000)
                rci, stop = C.c_int(0), C.c_int(0)
                check(L.preAlps_ECGInitializeMulti(C.byref(e), k, Bl.ctypes.data_as(pd), m, C.byref(rci)), "init")
                check(L.preAlps_BlockJacobiApply(e.R, e.P), "apply")
                check(L.preAlps_BlockOperator(e.P, e.AP), "product")
                hist = []
                while len(hist) < 1000:
                    check(L.preAlps_ECGIterate(C.byref(e), C.byref(rci)), "iterate")
                    if rci.value == 0:
                        check(L.preAlps_BlockOperator(e.P, e.AP), "product")
                        continue
                    check(L.preAlps_ECGStoppingCriterion(C.byref(e), C.byref(stop)), "stop")
                    g = np.zeros(k)
                    check(L.preAlps_ECGSystemResiduals(C.byref(e), g.ctypes.data_as(pd), None), "residuals")
                    hist.append(g)
                    if stop.value == 1:
                        break
                    check(L.preAlps_BlockJacobiApply(e.AP, e.Z), "apply")
                iters = e.iter
                x = np.zeros((m, k), order="F")
                check(L.preAlps_ECGFinalizeMulti(C.byref(e), x.ctypes.data_as(pd), m), "finalize")
                hists = gathered(np.array(hist).tobytes())
                assert iters == want.iters == len(hist), (iters, want.iters, len(hist))
                np.testing.assert_allclose(np.array(hist), want.sys_hist, rtol=1e-8)
                np.testing.assert_allclose(x, want.x, rtol=1e-8, atol=1e-8 * np.abs(want.x).max())
                assert all(h == hists[0] for h in hists), "the per-system norms differ between the ranks"

            case("caller's loop", callers_loop)

            # (6): no collective more per iteration than one system costs
            def collectives():
                b = prob.reference_rhs()
                count = {}
                for name, run in (("one", lambda it: prob.solve(b, T, tol=1e-12, max_iter=it)),
                                  ("four", lambda it: prob.solve_multi(G[lo:hi], T, tol=1e-12, max_iter=it))):
                    c = []
                    for it in (4, 12):
                        before = prob.stat("allreduces")
                        r = run(it)
                        assert r.iters == it, (name, r.iters, it)
                        c.append(prob.stat("allreduces") - before)
                    count[name] = (c[1] - c[0]) / 8.0
                print("rank", rank, "all-reduces per iteration", count, flush=True)
                assert count["one"] > 0 and count["four"] == count["one"], count

            case("collectives", collectives)

        prob.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok" if not fails else "fail: " + "\n".join(fails)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc())))


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_sharing_one_gpu_solve_several_systems_like_the_oracle(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] == "ok", r


def _loopback_worker(q):
    try:
        sys.path.insert(0, ROOT)
        import prealps_amd as pa
        from prealps_amd import gen
        rp, ci, v = gen.poisson3d_csr(N1)
        part, nparts = gen.box_partition(N1, BOX)
        prob = pa.EcgProblem(rp, ci, v, nparts, part, scale=True, device=0, shard=(1, 4))
        assert prob.m == N1 ** 3 // 4 and prob.stat("halo_rows") > 0
        B = np.random.default_rng(5).standard_normal((prob.m, 4))
        got = prob.solve_multi(B, T, tol=1e-12, max_iter=5)
        assert got.iters == 5 and len(got.res) == 5
        assert np.isfinite(got.res).all() and np.isfinite(got.sys_hist).all() and np.isfinite(got.x).all()
        np.testing.assert_allclose(got.sys_normb, np.linalg.norm(B, axis=0), rtol=1e-13)
        np.testing.assert_allclose((got.sys_hist ** 2).sum(axis=1), got.res ** 2, rtol=1e-12)
        warm = prob.solve_multi(B, T, tol=1e-12, max_iter=5, X0=got.x)
        assert np.isfinite(warm.res).all() and np.isfinite(warm.sys_res0).all() and (warm.sys_res0 > 0.0).all()
        prob.close()
        q.put("ok")
    except Exception as e:  # pragma: no cover
        import traceback
        q.put("fail: %s\n%s" % (e, traceback.format_exc()))


def _shard_of_one_worker(q):
    try:
        sys.path.insert(0, ROOT)
        import prealps_amd as pa
        from prealps_amd import gen
        rp, ci, v = gen.poisson3d_csr(N1)
        part, nparts = gen.box_partition(N1, BOX)
        B = np.random.default_rng(5).standard_normal((N1 ** 3, 4))
        got = {}
        for shard in (None, (0, 1)):       # (the shard last: the loopback hooks stay installed in the process)
            prob = pa.EcgProblem(rp, ci, v, nparts, part, scale=True, device=0, shard=shard)
            assert prob.m == N1 ** 3 and prob.stat("halo_rows") == 0
            # t = 4, Orthodir: the order of solve_first_step, for four systems and for two of two columns
            got[shard] = [prob.solve_multi(B[:, :k], T, tol=TOL) for k in (4, 2)]
            got[shard].append(prob.solve_multi(B, T, tol=TOL, X0=got[shard][0].x * (1.0 + 1e-3)))
            prob.close()
        for a, b in zip(got[(0, 1)], got[None]):
            print("shard (0, 1): iters", a.iters, b.iters, "res", a.res[-1], b.res[-1], flush=True)
            assert a.iters == b.iters > 0 and (a.sys_res <= TOL * a.sys_normb).all()
            assert a.res.tobytes() == b.res.tobytes() and a.sys_hist.tobytes() == b.sys_hist.tobytes()
            assert a.sys_normb.tobytes() == b.sys_normb.tobytes() and np.array_equal(a.x, b.x)
        q.put("ok")
    except Exception as e:  # pragma: no cover
        import traceback
        q.put("fail: %s\n%s" % (e, traceback.format_exc()))


def test_a_loopback_shard_of_a_group_of_one_is_the_single_process():
    """EcgProblem(..., shard=(0, 1)): the world size is 1, so the iteration is the one-process one (the solve-first order
    at t = 4 included) with its own per-system launch, and there is nothing to reduce: the same launches on the same
    data as without the shard, so the same bytes."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_shard_of_one_worker, args=(q,))
    p.start()
    res = q.get(timeout=240)
    p.join(timeout=60)
    assert res == "ok", res


def test_a_loopback_shard_runs_several_systems():
    """(7) EcgProblem(..., shard=(1, 4)): rank 1 of 4 rehearsed in one process, its collectives empty."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_loopback_worker, args=(q,))
    p.start()
    res = q.get(timeout=240)
    p.join(timeout=60)
    assert res == "ok", res
