"""The caller's own system on more than one rank: preAlps_ECGSolveSystem, preAlps_OperatorSystemResiduals and
preAlps_ECGSolveSystemRefined through EcgProblem.solve_system / system_residuals on a distributed problem.  Ranks share
the one GPU of the test box and talk through gloo, shaped like test_gpu_multi_rank_systems.py.  Every rank passes the
GLOBAL arrays (N rows in the caller's order and units), reads the rows it owns and returns them, zeros elsewhere.

The problem is Poisson 16^3 graded by S A0 S, S = diag(10^linspace(-2, 2, N)) -- the grading of test_gpu_system_solve.py,
so the caller's metric and the scaled one differ by two orders of magnitude -- in boxes of (4, 4, 8) with t = 4; the
right-hand sides are seeded standard-normal columns on the global rows.

The expected values come from the CPU oracle (oracle.ECG: the restated reference iteration), driven as
test_gpu_multi_rank_systems.py::_oracle_multi drives it and restated here: on P D A D P^T from b' = (d b)[perm], with
the stopping test ||(sum_c R(:, j s + c)) / dl|| <= tol ||b_j|| (dl = d[perm], ||b_j|| in the caller's units) or, for
stop="scaled", the per-system test on the scaled columns.  Tolerances against the oracle are those of
test_gpu_distributed.py::test_two_ranks_one_gpu_match_oracle; the recomputed ||b - A x|| / ||b|| on the original CSR is
held to 1.01 tol, the margin of test_gpu_system_solve.py::test_the_callers_tolerance_is_met_on_the_graded_problem.
On the CPU the oracle takes, at tol = 1e-5, ORACLE_ITERS iterations (original, scaled): 24 and 19 for k = 1, s = 4
Orthodir, 25 and 19 for k = 4, s = 1 Orthodir, 25 and 19 for k = 2, s = 2 Orthomin -- all far below max_iter, and the two
metrics differ (the scaled stop leaves a true relative residual of 21 to 111 tol); the workers assert both again
before they use a reference.

One spawn per process group; a worker makes one build and runs its cases on it (the numbers are the issue's):
  world 2: (1) k = 1, s = 4 and k = 4, s = 1, Orthodir; (2) k = 2, s = 2, Orthomin; (3) stop="scaled" is solve_multi on
           the same ranks in bits, and the scaled norms of stop="original" are those up to where the former stops;
           (4) a guess, system_residuals; (5) refusals reached together; (6) all-reduces per iteration; (7) refine=True
           on the fp32 operator; (8) device tensors.
  world 4: (1) with k = 4: every rank has more than one neighbour.
  one process: a preAlps_hip_loopback shard runs solve_system; shard=(0, 1) gives the bytes of the plain problem."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
MARGIN = 1.01             # test_the_callers_tolerance_is_met_on_the_graded_problem: recurrence against true residual
N1, BOX, T = 16, (4, 4, 8), 4
G_RANGE = (-2.0, 2.0)
MAX_ITER = 1000
# what the oracle takes on the CPU at TOL: (original, scaled)
ORACLE_ITERS = {(1, 4, "odir"): (24, 19), (4, 1, "odir"): (25, 19), (2, 2, "omin"): (25, 19)}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _matrix():
    from prealps_amd import gen
    rp, ci, v = gen.poisson3d_csr(N1)
    part, nparts = gen.box_partition(N1, BOX)
    return rp, ci, gen.graded_values(rp, ci, v, *G_RANGE), part, nparts


def _oracle_system(O, Bm, rowpos, Gp, dl, nbc, s, alg, metric, tol=TOL, max_iter=MAX_ITER):
    """The oracle's iteration on the scaled and permuted matrix Bm from R0 = the split of Gp = (d b)[perm]: system j in
    the columns j*s .. j*s + s - 1, a row of part p puts b'_j into column j*s + p % s.  metric "original": system j goes
    on while ||(sum_c R(:, j s + c)) / dl|| > tol * nbc[j] (nbc: ||b_j|| in the caller's units); "scaled": while the
    norm of its s columns exceeds tol * ||b'_j||.  x comes back in the library's space (N x k)."""
    N, k = Gp.shape
    t = k * s
    ref = O.ECG(Bm, rowpos, t, alg, O.NO_BS_RED, tol, max_iter)
    L, e = ref.L, ref.e
    rci, stop = C.c_int(0), C.c_int(0)
    assert L.orc_ecg_initialize(e, np.zeros(N), C.byref(rci)) == 0
    R = ref.panel(2, t)
    R[:] = 0.0
    for p in range(len(rowpos) - 1):
        for j in range(k):
            R[rowpos[p]:rowpos[p + 1], j * s + p % s] = Gp[rowpos[p]:rowpos[p + 1], j]
    nb = nbc if metric == "original" else np.linalg.norm(Gp, axis=0)
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
        Rk = np.asarray(ref.panel(2, t)).reshape(N, k, s)
        if metric == "original":
            g = np.linalg.norm(Rk.sum(axis=2) / dl[:, None], axis=0)
        else:
            g = np.sqrt((Rk ** 2).sum(axis=(0, 2)))
        res.append(L.orc_ecg_res(e))
        hist.append(g)
        if not (g > tol * nb).any() or L.orc_ecg_iter(e) >= max_iter:
            break
        L.orc_bj_apply(ref.bj.h, t, ptr(2) if alg == O.ORTHOMIN else ptr(1), N, ptr(3), N)
    x = np.asarray(ref.panel(4, t)).reshape(N, k, s).sum(axis=2)
    return dict(iters=L.orc_ecg_iter(e), res=np.array(res), hist=np.array(hist), x=x, nb=nb)


def _setting():
    """What the oracle needs of the graded problem, from the CSR alone: (A0, Bm, perm, rowpos, d, nparts)."""
    from oracle import oracle as O
    import scipy.sparse as sp
    rp, ci, vg, part, nparts = _matrix()
    N = N1 ** 3
    A0 = sp.csr_matrix((vg, ci, rp), shape=(N, N))
    Bm, perm, rowpos = O.permute_by_part(O.symrac_scale(A0), part, nparts)
    d = np.sqrt(1.0 / np.asarray(abs(A0).max(axis=1).todense()).ravel())
    return A0, Bm, np.asarray(perm), np.asarray(rowpos), d, nparts


def _rhs():
    return np.random.default_rng(20261020).standard_normal((N1 ** 3, 4))


def _reference(O, st, G, k, s, alg_name, metric, tol=TOL):
    A0, Bm, perm, rowpos, d, _ = st
    alg = O.ORTHODIR if alg_name == "odir" else O.ORTHOMIN
    Gk = G[:, :k]
    ref = _oracle_system(O, Bm, rowpos, (d[:, None] * Gk)[perm], d[perm], np.linalg.norm(Gk, axis=0), s, alg, metric, tol)
    x = np.empty_like(ref["x"])
    x[perm] = d[perm][:, None] * ref["x"]
    ref["x_caller"] = x
    return ref


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["LOCAL_RANK"] = "0"
        if world == 4:
            os.environ["PREALPS_HALO_OVERLAP"] = "1"
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import prealps_amd as pa
        from oracle import oracle as O
        rp, ci, vg, part, nparts = _matrix()
        prob = pa.EcgProblem(rp, ci, vg, nparts, part, scale=True, device=0, distributed=True)
        st = _setting()
        A0, Bm, perm, rowpos, d, _ = st
        N = N1 ** 3
        bounds = [int(rowpos[r * nparts // world]) for r in range(world + 1)]
        lo, hi = bounds[rank], bounds[rank + 1]
        own = prob.owned_rows
        assert prob.m == hi - lo and prob.stat("halo_rows") > 0
        np.testing.assert_array_equal(prob.perm, perm)
        np.testing.assert_array_equal(own, perm[lo:hi])
        np.testing.assert_allclose(prob.scaling, d, rtol=1e-15)
        others = np.ones(N, dtype=bool)
        others[own] = False
        G = _rhs()
        fails = []

        def gathered(obj):
            box = [None] * world
            dist.all_gather_object(box, obj)
            return box

        def assembled(x):
            assert not np.asarray(x)[others].any(), "a row this rank does not own is not zero"
            return sum(gathered(np.asarray(x)))

        def same_everywhere(got, what):
            for name in ("sys_hist", "sys_normb", "res"):
                box = gathered(getattr(got, name).tobytes())
                assert all(b == box[0] for b in box), "%s: %s differs between the ranks" % (what, name)
            box = gathered((got.iters, got.normb, got.sys_res_original.tobytes()))
            assert all(b == box[0] for b in box), "%s: iters, normb or sys_res differ between the ranks" % what

        def true_ratio(B, X):
            return np.linalg.norm(B - A0 @ X, axis=0) / np.linalg.norm(B, axis=0)

        def case(name, fn):
            try:
                fn()
            except Exception as e:
                import traceback
                fails.append("case %s: %s\n%s" % (name, e, traceback.format_exc()))

        cold = {}

        def against_oracle(k, s, alg_name):
            alg = pa.ORTHODIR if alg_name == "odir" else pa.ORTHOMIN
            B = np.asfortranarray(G[:, :k])
            ref = _reference(O, st, G, k, s, alg_name, "original")
            ref_s = _reference(O, st, G, k, s, alg_name, "scaled")
            # the reference is usable: it converges, and the two metrics do not stop together
            assert ref["iters"] < MAX_ITER and ref_s["iters"] < ref["iters"], (ref["iters"], ref_s["iters"])
            assert (ref["iters"], ref_s["iters"]) == ORACLE_ITERS[(k, s, alg_name)]
            got = cold[(k, s, alg_name)] = prob.solve_system(B, k * s, stop="original", ortho_alg=alg, tol=TOL, max_iter=MAX_ITER)
            X = assembled(got.x)
            ratio = true_ratio(B, X)
            print("rank", rank, "world", world, (k, s, alg_name), "iters", got.iters, ref["iters"], "res", got.res[-1],
                  ref["res"][-1], "sys / oracle - 1", got.sys_hist[-1] / ref["hist"][-1] - 1.0, "true ratio / tol",
                  ratio / TOL, flush=True)
            assert got.metric == "original" and got.x.shape == (N, k) and got.sys_hist.shape == (got.iters, k)
            assert got.iters == ref["iters"], (got.iters, ref["iters"])
            np.testing.assert_allclose(got.res, ref["res"], rtol=1e-8)
            np.testing.assert_allclose(got.sys_hist[-1], ref["hist"][-1], rtol=1e-6)
            np.testing.assert_allclose(X, ref["x_caller"], rtol=1e-7, atol=1e-9 * np.abs(ref["x_caller"]).max())
            np.testing.assert_allclose(got.sys_normb, np.linalg.norm(B, axis=0), rtol=1e-13)
            assert (got.sys_res <= TOL * got.sys_normb).all()
            assert got.sys_res_original.tobytes() == got.sys_hist[-1].tobytes()      # the bits of the last stopping test
            same_everywhere(got, str((k, s, alg_name)))
            assert (ratio <= MARGIN * TOL).all(), ratio / TOL
            # rows of x a rank does not own keep their bits: a sentinel-filled host array through the C entry
            sentinel = -12345.678
            x = np.full((N, k), sentinel, order="F")
            e = prob.new_ecg(k * s, alg, pa.NO_BS_RED, TOL, MAX_ITER)
            nh = C.c_int(0)
            from prealps_amd.lib import check, SYS_STOP_ORIGINAL
            check(prob.L.preAlps_ECGSolveSystem(C.byref(e), k, B.ctypes.data, N, None, 0, x.ctypes.data, N, SYS_STOP_ORIGINAL,
                                                None, None, None, None, None, 0, C.byref(nh)), "preAlps_ECGSolveSystem")
            assert (x[others] == sentinel).all(), "a row this rank does not own was written"
            assert x[own].tobytes() == np.asarray(got.x)[own].tobytes()

        # (1)
        if world == 2:
            case("k = 1, s = 4", lambda: against_oracle(1, 4, "odir"))
        case("k = 4, s = 1", lambda: against_oracle(4, 1, "odir"))

        if world == 2:
            # (2)
            case("k = 2, s = 2, Orthomin", lambda: against_oracle(2, 2, "omin"))

            # (3) stop="scaled" is solve_multi on the same ranks; the scaled norms of stop="original" are its norms
            def scaled(k, s):
                B = G[:, :k]
                sc = prob.solve_system(B, k * s, stop="scaled", tol=TOL)
                mu = prob.solve_multi((d[:, None] * B)[perm][lo:hi], k * s, tol=TOL)
                orig = cold[(k, s, "odir")] if (k, s, "odir") in cold else prob.solve_system(B, k * s, stop="original", tol=TOL)
                back = np.zeros((N, k))
                back[own] = d[own][:, None] * mu.x.reshape(hi - lo, k)
                n = sc.iters
                print("rank", rank, "scaled", (k, s), "iters", sc.iters, mu.iters, "original", orig.iters, flush=True)
                assert sc.iters == mu.iters > 0 and sc.res.tobytes() == mu.res.tobytes()
                assert sc.sys_hist.tobytes() == mu.sys_hist.tobytes() and sc.normb == mu.normb
                assert np.asarray(sc.x).tobytes() == back.tobytes()
                assert orig.iters > sc.iters
                assert orig.res[:n].tobytes() == sc.res[:n].tobytes()
                same_everywhere(sc, "scaled %s" % ((k, s),))

            case("scaled 2 x 2", lambda: scaled(2, 2))
            case("scaled 1 x 4", lambda: scaled(1, 4))

            # (4) a guess
            def guess():
                first = cold[(4, 1, "odir")]
                X0 = assembled(prob.solve_system(G, T, stop="original", tol=1e-3).x)
                warm = prob.solve_system(G, T, x0=X0, tol=TOL)
                zero = prob.solve_system(G, T, x0=np.zeros((N, 4)), tol=TOL)
                tight = assembled(prob.solve_system(G, T, tol=1e-8).x)
                done = prob.solve_system(G, T, x0=tight, tol=TOL)
                res, nb = prob.system_residuals(G, X0)
                r0 = np.linalg.norm(G - A0 @ X0, axis=0)
                print("rank", rank, "guess iters", warm.iters, "cold", first.iters, "system_residuals / scipy - 1",
                      res / r0 - 1.0, flush=True)
                assert 0 < warm.iters < first.iters, (warm.iters, first.iters)
                assert (warm.sys_res <= TOL * warm.sys_normb).all()
                assert (true_ratio(G, assembled(warm.x)) <= MARGIN * TOL).all()
                assert zero.iters == first.iters and zero.res.tobytes() == first.res.tobytes()
                assert zero.sys_hist.tobytes() == first.sys_hist.tobytes()
                assert np.asarray(zero.x).tobytes() == np.asarray(first.x).tobytes()
                assert done.iters == 0 and len(done.res) == 0
                assert np.asarray(done.x)[own].tobytes() == tight[own].tobytes() and not np.asarray(done.x)[others].any()
                np.testing.assert_allclose(res, r0, rtol=1e-10)
                np.testing.assert_allclose(nb, np.linalg.norm(G, axis=0), rtol=1e-13)
                box = gathered((res.tobytes(), nb.tobytes()))
                assert all(b == box[0] for b in box), "system_residuals differs between the ranks"
                same_everywhere(warm, "warm")

            case("guess", guess)

            # (5) refusals that both ranks reach
            def refusals():
                own0 = perm[bounds[0]:bounds[1]]
                own1 = perm[bounds[1]:bounds[2]]
                Gn = G.copy()
                Gn[own0[len(own0) // 2], 1] = np.nan          # a row only rank 0 owns
                with pytest.raises(pa.PreAlpsError, match="preAlps_ECGSolveSystem.*right-hand side 1.*not finite"):
                    prob.solve_system(Gn, T, tol=TOL)
                Gz = G.copy()
                Gz[own1, 2] = 0.0                              # zero on rank 1's rows only: its global norm is not zero
                got = prob.solve_system(Gz, T, tol=TOL)
                ref = _reference(O, st, Gz, 4, 1, "odir", "original")
                print("rank", rank, "locally zero rhs iters", got.iters, ref["iters"], flush=True)
                assert got.iters == ref["iters"], (got.iters, ref["iters"])
                np.testing.assert_allclose(got.sys_normb, np.linalg.norm(Gz, axis=0), rtol=1e-13)
                Gz[:, 2] = 0.0
                with pytest.raises(pa.PreAlpsError, match="preAlps_ECGSolveSystem.*right-hand side 2 has norm zero"):
                    prob.solve_system(Gz, T, tol=TOL)
                with pytest.raises(pa.PreAlpsError, match="preAlps_ECGSolveSystem.*ADAPT_BS.*single process"):
                    prob.solve_system(G, T, bs_red=pa.ADAPT_BS, tol=TOL)
                # ... and the ranks are together afterwards
                again = prob.solve_system(G, T, tol=TOL)
                assert again.res.tobytes() == cold[(4, 1, "odir")].res.tobytes()
                assert np.asarray(again.x).tobytes() == np.asarray(cold[(4, 1, "odir")].x).tobytes()

            case("refusals", refusals)

            # (6) the caller's metric costs no collective more per iteration than preAlps_ECGSolve
            def collectives(lazy):
                if not lazy:
                    os.environ["PREALPS_ECG_LAZY_STOP"] = "0"
                try:
                    b = prob.reference_rhs()
                    count = {}
                    for name, run in (("solve", lambda it: prob.solve(b, T, tol=1e-12, max_iter=it)),
                                      ("one", lambda it: prob.solve_system(G[:, 0], T, tol=1e-12, max_iter=it)),
                                      ("four", lambda it: prob.solve_system(G, T, tol=1e-12, max_iter=it))):
                        c = []
                        for it in (4, 12):
                            before = prob.stat("allreduces")
                            r = run(it)
                            assert r.iters == it, (name, r.iters, it)
                            c.append(prob.stat("allreduces") - before)
                        count[name] = (c[1] - c[0]) / 8.0
                finally:
                    os.environ.pop("PREALPS_ECG_LAZY_STOP", None)
                print("rank", rank, "lazy" if lazy else "eager", "all-reduces per iteration", count, flush=True)
                assert count["solve"] > 0 and count["one"] == count["four"] == count["solve"], count

            case("collectives, lazy stopping test", lambda: collectives(True))
            case("collectives, eager stopping test", lambda: collectives(False))

            # ... and the eager test, where the sums ride in the all-reduce of the norm itself, gives the same solve
            def eager():
                os.environ["PREALPS_ECG_LAZY_STOP"] = "0"
                try:
                    got = prob.solve_system(G, T, tol=TOL)
                finally:
                    del os.environ["PREALPS_ECG_LAZY_STOP"]
                first = cold[(4, 1, "odir")]
                assert got.iters == first.iters
                np.testing.assert_allclose(got.sys_hist, first.sys_hist, rtol=1e-8)
                same_everywhere(got, "eager")

            case("eager", eager)

            # (8) device tensors give the bits of the host path
            def device():
                first = cold[(2, 2, "omin")]
                tb = torch.from_numpy(np.ascontiguousarray(G[:, :2])).to("cuda:0")
                got = prob.solve_system(tb, T, ortho_alg=pa.ORTHOMIN, tol=TOL)
                assert got.x.is_cuda and got.iters == first.iters
                assert got.x.cpu().numpy().tobytes() == np.ascontiguousarray(first.x).tobytes()
                assert got.res.tobytes() == first.res.tobytes() and got.sys_hist.tobytes() == first.sys_hist.tobytes()
                tx = torch.from_numpy(np.ascontiguousarray(assembled(first.x))).to("cuda:0")
                rd, nd = prob.system_residuals(tb, tx)
                rh, nh_ = prob.system_residuals(G[:, :2], assembled(first.x))
                assert rd.tobytes() == rh.tobytes() and nd.tobytes() == nh_.tobytes()
                # a converged guess on the device: the owned rows of the guess, bit for bit, zeros elsewhere
                tight = assembled(prob.solve_system(G[:, :2], T, tol=1e-8).x)
                tt = torch.from_numpy(np.ascontiguousarray(tight)).to("cuda:0")
                done = prob.solve_system(tb, T, x0=tt, tol=TOL)
                dx = done.x.cpu().numpy()
                assert done.iters == 0 and dx[own].tobytes() == tight[own].tobytes() and not dx[others].any()

            case("device", device)

            # (7) the refined solve on the fp32 operator reaches the caller's tolerance on the fp64 matrix
            def refined():
                tol = 1e-9
                prob.set_operator_precision("single")
                try:
                    plain = prob.solve_system(G[:, :2], T, tol=tol)
                    bits = prob.stat("spmm_precision")
                    got = prob.solve_system(G[:, :2], T, tol=tol, refine=True, max_passes=6)
                finally:
                    prob.set_operator_precision("double")
                X = assembled(got.x)
                ratio = true_ratio(G[:, :2], X)
                box = gathered((got.passes, got.refine_status, got.pass_iters.tobytes(), got.pass_res.tobytes(), got.iters))
                ra = true_ratio(G[:, :2], assembled(plain.x))
                print("rank", rank, "refined: storage", bits, "plain true ratio / tol", ra / tol, "passes", got.passes,
                      got.refine_status, "iters", got.pass_iters, "true ratio / tol", ratio / tol, flush=True)
                assert all(b == box[0] for b in box), "the passes differ between the ranks"
                assert got.passes >= 1 and got.refine_status == "converged", (got.passes, got.refine_status)
                if np.any(ra > tol):          # (as test_gpu_refined_solve.py: one pass would not have done)
                    assert got.passes >= 2
                assert got.pass_iters[0] == plain.iters
                assert (ratio <= MARGIN * tol).all(), ratio / tol

            case("refined", refined)

        prob.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok" if not fails else "fail: " + "\n".join(fails)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc())))


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_sharing_one_gpu_solve_the_callers_system_like_the_oracle(world):
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


def _one_process_worker(q):
    try:
        sys.path.insert(0, ROOT)
        import prealps_amd as pa
        rp, ci, vg, part, nparts = _matrix()
        N = N1 ** 3
        B = _rhs()
        got = {}
        for shard in (None, (0, 1)):       # (the shards last: the loopback hooks stay installed in the process)
            prob = pa.EcgProblem(rp, ci, vg, nparts, part, scale=True, device=0, shard=shard)
            assert prob.m == N and len(prob.owned_rows) == N
            got[shard] = [prob.solve_system(B[:, :k], T, stop=stop, tol=TOL) for k, stop in ((4, "original"), (1, "original"), (2, "scaled"))]
            got[shard].append(prob.solve_system(B, T, x0=got[shard][0].x * (1.0 + 1e-3), tol=TOL))
            got[shard].append(prob.system_residuals(B, got[shard][0].x))
            prob.close()
        for a, b in zip(got[(0, 1)][:4], got[None][:4]):
            print("shard (0, 1): iters", a.iters, b.iters, "res", a.res[-1], b.res[-1], flush=True)
            assert a.iters == b.iters > 0
            assert a.res.tobytes() == b.res.tobytes() and a.sys_hist.tobytes() == b.sys_hist.tobytes()
            assert a.sys_normb.tobytes() == b.sys_normb.tobytes() and a.x.tobytes() == b.x.tobytes()
            assert a.sys_res_original.tobytes() == b.sys_res_original.tobytes()
        for a, b in zip(got[(0, 1)][4], got[None][4]):
            assert a.tobytes() == b.tobytes()
        # rank 1 of 4 rehearsed in one process, its collectives empty
        prob = pa.EcgProblem(rp, ci, vg, nparts, part, scale=True, device=0, shard=(1, 4))
        own = prob.owned_rows
        assert prob.m == N // 4 == len(own) and prob.stat("halo_rows") > 0
        others = np.ones(N, dtype=bool)
        others[own] = False
        run = prob.solve_system(B[:, 0], T, tol=1e-12, max_iter=5)
        assert run.iters == 5 and len(run.res) == 5 and run.x.shape == (N,)
        assert np.isfinite(run.res).all() and np.isfinite(run.sys_hist).all() and np.isfinite(run.x).all()
        assert run.x[own].any() and not run.x[others].any()
        np.testing.assert_allclose(run.sys_normb, [np.linalg.norm(B[own, 0])], rtol=1e-13)      # (its share: nothing is reduced)
        res, nb = prob.system_residuals(B[:, :2], np.zeros((N, 2)))
        np.testing.assert_allclose(res, nb, rtol=1e-13)
        prob.close()
        q.put("ok")
    except Exception as e:  # pragma: no cover
        import traceback
        q.put("fail: %s\n%s" % (e, traceback.format_exc()))


def test_loopback_shards_run_the_callers_system_in_one_process():
    """EcgProblem(..., shard=(1, 4)).solve_system(b, 4, max_iter=5) runs and writes the rows it owns and no other;
    shard=(0, 1), a group of one, gives the bytes of the plain one-process solve_system."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_process_worker, args=(q,))
    p.start()
    res = q.get(timeout=240)
    p.join(timeout=60)
    assert res == "ok", res
