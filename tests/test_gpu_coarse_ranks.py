"""Two-level block Jacobi on several processes: M^-1 = B^-1 + Z E^-1 Z^T with a coarse space attached collectively
(preAlps_BlockJacobiSetCoarseSpace on a distributed problem).  Ranks share the one GPU of the test box and talk through
gloo, shaped like test_gpu_system_ranks.py: one spawn per process group.

Problem: elasticity 12 x 10 x 10 in 150 boxes, t = 4, the three translations (k = 3).  Every worker holds the global CSR
and builds the references globally in NumPy from it, d, perm, rowpos and the aggregates: A' = P D A D P^T, Z, E = Z^T A' Z
and inv(E); the solve is compared with the restatement of Orthodir with M^-1 as a callable (restated here from
test_gpu_coarse_space.py).  The bound of the apply and the projection is that file's: 100 nc eps cond_2(E), relative to
the coarse term.

  world 2: (1) apply against NumPy at strides 4, 8 and 16 (13 live columns), default aggregates and hand-made ones of
           2-3 parts with one spanning the rank boundary, dead columns, two applies in bits; (2) projection; (3) solve
           against the restatement, fewer iterations than the plain solve, identical histories; (4) all-reduce count;
           (5) a values update ("keep", "refactor", against a fresh problem -- the worker's second build, at its end);
           (6) refusals reached together, clear_coarse_space.
  world 4: (1) at stride 4 and (3), default aggregates: every rank has more than one neighbour.
  one process: a preAlps_hip_loopback shard still refuses set_coarse_space."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
TOL = 1e-5
NN, BOX, T, K = (12, 10, 10), (2, 2, 2), 4, 3
# what the restatement takes on one process for the right-hand side of _rhs(): with the coarse space, with block Jacobi alone
RESTATED = (28, 49)
SENTINEL = -12345.678


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _matrix():
    from prealps_amd import gen
    rp, ci, v = gen.elasticity3d_csr(NN)
    part, nparts = gen.box_partition_nodes(NN, BOX)
    return rp, ci, v, part, nparts


def _new_values(rp, ci, v):
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    rows = np.repeat(np.arange(N), np.diff(rp))
    return s[rows] * v * s[ci]


def _rhs(N):
    return np.random.default_rng(20261019).standard_normal((N, 2))


def _internal(rp, ci, v, perm):
    """A' = P D A D P^T and d from the CSR alone (d_i = sqrt(1 / max_j |a_ij|), perm[new] = old)."""
    import scipy.sparse as sp
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    d = np.sqrt(1.0 / np.asarray(abs(A).max(axis=1).todense()).ravel())
    D = sp.diags(d)
    Ap = sp.csr_matrix((D @ A @ D)[perm][:, perm])
    Ap.sort_indices()
    return Ap, d


def _numpy_coarse(Ap, d, perm, rowpos, V, aggr):
    import scipy.sparse as sp
    Vp = (V / d[:, None])[perm]
    N, k = Vp.shape
    g = np.repeat(np.asarray(aggr), np.diff(rowpos))
    rows = np.repeat(np.arange(N), k)
    cols = (g[:, None] * k + np.arange(k)[None, :]).ravel()
    Z = sp.csr_matrix((Vp.ravel(), (rows, cols)), shape=(N, (int(np.max(aggr)) + 1) * k))
    E = (Z.T @ Ap @ Z).toarray()
    return Z, E, np.linalg.inv(E)


def _split(V, rowpos, s):
    N, k = V.shape
    out = np.zeros((N, k * s))
    for p in range(len(rowpos) - 1):
        for j in range(k):
            out[rowpos[p]:rowpos[p + 1], j * s + p % s] = V[rowpos[p]:rowpos[p + 1], j]
    return out


def _restate(A, rowpos, precond, B, s, tol=TOL, max_iter=600):
    """The ECG Orthodir iteration on R0 = the split of the k columns of B into s columns each, with M^-1 = precond
    (test_gpu_coarse_space.py::_restate).  Returns the per-system residual history (iterations x k)."""
    N, k = B.shape
    t = k * s
    X, R = np.zeros((N, t)), _split(B, rowpos, s)
    nb = np.linalg.norm(B, axis=0)
    Pm, Pp, APp = precond(R), np.zeros((N, t)), np.zeros((N, t))
    hist = []
    for _ in range(max_iter):
        AP = A @ Pm
        U = np.linalg.cholesky(Pm.T @ AP).T
        Pm, AP = np.linalg.solve(U.T, Pm.T).T, np.linalg.solve(U.T, AP.T).T
        alpha = Pm.T @ R
        X += Pm @ alpha
        R -= AP @ alpha
        g = np.sqrt((R ** 2).reshape(N, k, s).sum(axis=(0, 2)))
        hist.append(g)
        if not (g > tol * nb).any():
            break
        Z = precond(AP)
        Z -= np.hstack([Pm, Pp]) @ (np.hstack([AP, APp]).T @ Z)
        Pp, APp, Pm = Pm, AP, Z
    return np.array(hist)


def _preconditioners(Ap, rowpos, Z, Einv):
    inv = [np.linalg.inv(Ap[r0:r1, r0:r1].toarray()) for r0, r1 in zip(rowpos[:-1], rowpos[1:])]

    def plain(X):
        Y = np.empty_like(X)
        for p in range(len(inv)):
            Y[rowpos[p]:rowpos[p + 1]] = inv[p] @ X[rowpos[p]:rowpos[p + 1]]
        return Y

    return plain, lambda X: plain(X) + Z @ (Einv @ (Z.T @ X))


def _spanning(nparts, cuts):
    """Aggregates of two or three consecutive parts, numbered without gaps, one of which spans a rank boundary."""
    for s in range(3):
        aggr = ((np.arange(nparts) + s) // 3).astype(np.int32)
        if any(aggr[c - 1] == aggr[c] for c in cuts[1:-1]):
            return aggr
    raise AssertionError("no shift makes an aggregate span a boundary")


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["LOCAL_RANK"] = "0"
        if world == 4:
            os.environ["PREALPS_HALO_OVERLAP"] = "1"
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import prealps_amd as pa
        from prealps_amd.nearkernel import translations
        rp, ci, v, part, nparts = _matrix()
        N = len(rp) - 1
        prob = pa.EcgProblem(rp, ci, v, nparts, part, scale=True, device=0, distributed=True)
        prob.create_block_jacobi()
        L = prob.L
        L.pa_rt_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.pa_rt_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        perm, rowpos = np.asarray(prob.perm), np.asarray(prob.rowpos, dtype=np.int64)
        cuts = [r * nparts // world for r in range(world + 1)]
        lo, hi = int(rowpos[cuts[rank]]), int(rowpos[cuts[rank + 1]])
        assert prob.m == hi - lo and prob.stat("halo_rows") > 0 and prob.nparts == nparts == 150
        Ap, d = _internal(rp, ci, v, perm)
        np.testing.assert_allclose(prob.scaling, d, rtol=1e-15)
        V = np.asfortranarray(translations(N, K))
        fails = []

        def gathered(obj):
            box = [None] * world
            dist.all_gather_object(box, obj)
            return box

        def case(name, fn):
            import time
            t0 = time.perf_counter()
            try:
                fn()
            except Exception as e:
                import traceback
                fails.append("case %s: %s\n%s" % (name, e, traceback.format_exc()))
            print("rank %d of %d: case %s took %.2f s" % (rank, world, name, time.perf_counter() - t0), flush=True)

        def apply(W, t):
            return prob.block_jacobi_apply(np.ascontiguousarray(W[lo:hi]), t)

        def raw_apply(W, t):
            """The whole m x t output panel of an apply on the live columns of W; the dead columns of the input hold
            garbage, those of the output a sentinel beforehand."""
            n = W.shape[1]
            dx, dy = prob.panel(n, t), prob.panel(n, t)
            try:
                hin = np.full((prob.m, t), 7.0e7)
                hin[:, :n] = W[lo:hi]
                hout = np.full((prob.m, t), SENTINEL)
                assert L.pa_rt_h2d(dx.val, hin.ctypes.data, hin.nbytes) == 0 and L.pa_rt_h2d(dy.val, hout.ctypes.data, hout.nbytes) == 0
                pa.lib.check(L.preAlps_BlockJacobiApply(C.byref(dx), C.byref(dy)), "preAlps_BlockJacobiApply")
                prob.sync()
                assert L.pa_rt_d2h(hout.ctypes.data, dy.val, hout.nbytes) == 0
                return hout
            finally:
                prob.panel_free(dx)
                prob.panel_free(dy)

        rng = np.random.default_rng(77)                          # the same global arrays on every rank
        strides = (4, 8, 16) if world == 2 else (4,)
        W = {t: rng.standard_normal((N, t if t < 16 else 13)) for t in strides}
        plain = {t: apply(W[t], t) for t in strides}
        plain_raw = raw_apply(W[16], 16) if 16 in strides else None
        W4 = rng.standard_normal((N, 4))
        plain4 = apply(W4, 4)
        w_proj = {}

        # (1) + (2)
        def apply_and_projection(mode):
            want_aggr = np.arange(nparts, dtype=np.int32) if mode == "default" else _spanning(nparts, cuts)
            Z, E, Einv = _numpy_coarse(Ap, d, perm, rowpos, V, want_aggr)
            nc = E.shape[0]
            # the plain apply of A' Z w, taken before the attach
            prob.clear_coarse_space()
            w = w_proj.setdefault(mode, np.random.default_rng(5 + nc).standard_normal((nc, T)))
            Zw = Z @ w
            AZw = Ap @ Zw
            plain_AZw = apply(AZw, T)
            prob.set_coarse_space(V, None if mode == "default" else want_aggr)
            aggr = prob.coarse_aggregates()
            assert np.array_equal(aggr, want_aggr) and len(aggr) == nparts
            box = gathered(aggr.tobytes())
            assert all(b == box[0] for b in box)
            mine = np.unique(aggr[cuts[rank]:cuts[rank + 1]])
            assert prob.stat("bj_coarse_dofs") == nc and prob.stat("bj_coarse_aggregates") == aggr.max() + 1
            # the bytes are the rank's own: its rows of the inverse, not all of them (at nc = 450 the inverse outweighs the rest)
            assert prob.stat("bj_coarse_bytes") > 8 * len(mine) * K * nc
            if mode == "default":
                assert prob.stat("bj_coarse_bytes") < 8 * nc * nc
            cond = np.linalg.cond(E)
            bound = 100 * nc * EPS * cond
            n0 = prob.stat("bj_coarse_applies")
            for t in strides:
                got = apply(W[t], t)
                coarse = (Z @ (Einv @ (Z.T @ W[t])))[lo:hi]
                err = np.linalg.norm(got - (plain[t] + coarse)) / np.linalg.norm(coarse)
                print("rank %d of %d, %s aggregates, nc %d, cond_2(E) %.3e: stride %2d apply error %.3e, bound %.3e"
                      % (rank, world, mode, nc, cond, t, err, bound), flush=True)
                assert err <= bound
                assert got.tobytes() == apply(W[t], t).tobytes()                 # two applies agree in bits
            assert prob.stat("bj_coarse_applies") == n0 + 2 * len(strides)
            if plain_raw is not None:                                               # dead columns keep their bits
                raw = raw_apply(W[16], 16)
                assert raw[:, 13:].tobytes() == plain_raw[:, 13:].tobytes()
                assert raw[:, :13].tobytes() == np.ascontiguousarray(apply(W[16], 16)).tobytes()
            got = apply(AZw, T) - plain_AZw
            err = np.linalg.norm(got - Zw[lo:hi]) / np.linalg.norm(Zw[lo:hi])
            print("rank %d of %d, %s aggregates: projection error %.3e, bound %.3e" % (rank, world, mode, err, bound), flush=True)
            assert err <= bound

        if world == 2:
            case("apply, hand-made aggregates", lambda: apply_and_projection("spanning"))
        case("apply, default aggregates", lambda: apply_and_projection("default"))

        Bi = _rhs(N)
        state = {}

        # (3)
        def solve():
            prob.clear_coarse_space()
            plain_run = prob.solve_multi(Bi[lo:hi, :1], T, tol=TOL)
            prob.set_coarse_space(V)
            aggr = prob.coarse_aggregates()
            Z, E, Einv = _numpy_coarse(Ap, d, perm, rowpos, V, aggr)
            p_plain, p_coarse = _preconditioners(Ap, rowpos, Z, Einv)
            hist = _restate(Ap, rowpos, p_coarse, Bi[:, :1], T)
            hist_plain = _restate(Ap, rowpos, p_plain, Bi[:, :1], T)
            assert (len(hist), len(hist_plain)) == RESTATED, (len(hist), len(hist_plain))
            got = prob.solve_multi(Bi[lo:hi, :1], T, tol=TOL)
            print("rank %d of %d: iterations to %g: block Jacobi %d, with the coarse space %d (restatement %d and %d)"
                  % (rank, world, TOL, plain_run.iters, got.iters, len(hist_plain), len(hist)), flush=True)
            assert abs(got.iters - len(hist)) <= 1
            np.testing.assert_allclose(got.sys_hist[:8, 0], hist[:8, 0], rtol=1e-8)
            assert got.iters < plain_run.iters
            box = gathered((got.iters, got.sys_hist.tobytes(), got.res.tobytes()))
            assert all(b == box[0] for b in box), "the histories differ between the ranks"
            state["iters"] = got.iters

        case("solve", solve)

        if world == 2:
            # (4) one all-reduce per coarse apply on top of the plain solve's, and nothing else
            def collectives():
                b = Bi[lo:hi, :1]
                prob.clear_coarse_space()
                base = {}
                for it in (4, 12):
                    before = prob.stat("allreduces")
                    assert prob.solve_multi(b, T, tol=1e-12, max_iter=it).iters == it
                    base[it] = prob.stat("allreduces") - before
                prob.set_coarse_space(V)
                for it in (4, 12):
                    before, a0 = prob.stat("allreduces"), prob.stat("bj_coarse_applies")
                    assert prob.solve_multi(b, T, tol=1e-12, max_iter=it).iters == it
                    grown, applies = prob.stat("allreduces") - before, prob.stat("bj_coarse_applies") - a0
                    print("rank %d: %d iterations: %d all-reduces, %d without the coarse space, %d coarse applies"
                          % (rank, it, grown, base[it], applies), flush=True)
                    assert applies >= it and grown == base[it] + applies
                assert (base[12] - base[4]) % 8 == 0 and base[12] > base[4]

            case("collectives", collectives)

            # (6) refusals reached together
            def refusals():
                prob.set_coarse_space(V)
                before = apply(W4, T)
                addr = prob.stat("bj_coarse_einv_address")
                Vn = V.copy(order="F")
                if rank == 1:
                    Vn[perm[lo + 5], 1] = np.nan                                     # on one rank only
                with pytest.raises(pa.PreAlpsError, match="preAlps_BlockJacobiSetCoarseSpace.*(not finite|another process)") as ei:
                    prob.set_coarse_space(Vn)
                assert ("not finite" in str(ei.value)) == (rank == 1)
                assert prob.stat("bj_coarse_einv_address") == addr and apply(W4, T).tobytes() == before.tobytes()
                Vd = V.copy(order="F")
                Vd[:, 1] = Vd[:, 0]                                                  # a duplicated vector: E is singular
                with pytest.raises(pa.PreAlpsError, match="aggregate 0, vector 1"):
                    prob.set_coarse_space(Vd)
                assert prob.stat("bj_coarse_einv_address") == addr and prob.stat("bj_coarse_dofs") == 450
                assert apply(W4, T).tobytes() == before.tobytes()
                assert not np.array_equal(before, plain4)
                prob.clear_coarse_space()
                assert prob.stat("bj_coarse_dofs") == 0
                assert apply(W4, T).tobytes() == plain4.tobytes()                   # the plain apply in bits

            case("refusals", refusals)

            # (5) a values update
            def values():
                v2 = _new_values(rp, ci, v)
                b = Bi[lo:hi, :1]
                prob.set_coarse_space(V)
                addr = prob.stat("bj_coarse_einv_address")
                prob.update_values(v2, precond="keep")                                # lagged factor and coarse space
                lag = prob.solve_multi(b, T, tol=TOL)
                assert (lag.sys_res <= TOL * lag.sys_normb).all() and prob.stat("bj_coarse_builds") == 1
                prob.update_values(v2, precond="refactor")
                assert prob.stat("bj_coarse_builds") == 2 and prob.stat("bj_coarse_einv_address") == addr
                state["refactor"] = prob.solve_multi(b, T, tol=TOL)
                state["refactor_apply"] = apply(W4, T)
                prob.update_values(v2, precond="rebuild")                             # attached again to the new factor
                assert prob.stat("bj_coarse_builds") == 1 and prob.stat("bj_coarse_dofs") == 450
                assert prob.solve_multi(b, T, tol=TOL).iters == state["refactor"].iters
                print("rank %d: iterations after a values update: lagged %d, refactored %d" % (rank, lag.iters, state["refactor"].iters),
                      flush=True)

            case("values", values)

        prob.close()
        if world == 2 and "refactor" in state:
            def fresh_values():
                v2 = _new_values(rp, ci, v)
                fresh = pa.EcgProblem(rp, ci, v2, nparts, part, scale=True, device=0, distributed=True)
                try:
                    fresh.create_block_jacobi(coarse=V)
                    run = fresh.solve_multi(Bi[lo:hi, :1], T, tol=TOL)
                    out = fresh.block_jacobi_apply(np.ascontiguousarray(W4[lo:hi]), T)
                finally:
                    fresh.close()
                print("rank %d: a fresh problem on the new values: %d iterations" % (rank, run.iters), flush=True)
                assert run.iters == state["refactor"].iters
                assert out.tobytes() == state["refactor_apply"].tobytes()

            case("values, fresh problem", fresh_values)
        dist.barrier()
        dist.destroy_process_group()
        for f in fails:
            print("rank %d: %s" % (rank, f), flush=True)
        q.put((rank, "ok" if not fails else "fail: " + "\n".join(fails)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc())))


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_sharing_one_gpu_apply_and_solve_with_the_coarse_space(world):
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
        from prealps_amd.nearkernel import translations
        rp, ci, v, part, nparts = _matrix()
        N = len(rp) - 1
        prob = pa.EcgProblem(rp, ci, v, nparts, part, scale=True, device=0, shard=(1, 4))
        try:
            prob.create_block_jacobi()
            W = np.random.default_rng(3).standard_normal((prob.m, T))
            before = prob.block_jacobi_apply(W, T)
            with pytest.raises(pa.PreAlpsError, match="preAlps_BlockJacobiSetCoarseSpace.*preAlps_hip_loopback") as ei:
                prob.set_coarse_space(translations(N, K))
            assert "one process" not in str(ei.value)
            assert prob.stat("bj_coarse_dofs") == 0 and prob.block_jacobi_apply(W, T).tobytes() == before.tobytes()
        finally:
            prob.close()
        q.put("ok")
    except Exception as e:  # pragma: no cover
        import traceback
        q.put("fail: %s\n%s" % (e, traceback.format_exc()))


def test_a_loopback_shard_still_refuses_the_coarse_space():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_loopback_worker, args=(q,))
    p.start()
    res = q.get(timeout=240)
    p.join(timeout=60)
    assert res == "ok", res
