"""The solution history on more than one rank: preAlps_SolutionHistory* and preAlps_ECGSolveSystemHistory through
EcgProblem on a distributed problem.  Ranks share the one GPU of the test box and talk through gloo, shaped like
tests/test_gpu_system_ranks.py: one spawn per process group, a worker runs its cases one after the other.  Every rank
passes the GLOBAL arrays (N rows in the caller's order and units), reads the rows it owns and returns them, zeros
elsewhere; the ring holds the owned rows of every solution.

Problems, as tests/test_gpu_solution_history.py builds them: P = Poisson 10^3 with part[i] = (i // 5) % 8 (a rank's
rows are scattered, the row map is far from the identity, every rank has neighbours); G = the graded S A0 S on 8
contiguous parts with its second grading G_RANGE_2; H = the heat matrix of tests/history_ref.py on its 8 parts.
Right-hand sides: default_rng(20260407).standard_normal((N, 16)).  Bounds and references: tests/history_ref.py; they
hold for any order of summation, so a sum formed per rank and then reduced stays inside them.

  world 2: (1) Galerkin; (2) the bits of the solve; (3) a repeated right-hand side; (4) capacity 3, five appends;
           (5) a values update; (6) the heat sequence; (7) all-reduces per entry; (8) refusals reached together.
  world 4: (1), (2) and (6).
  one process: a preAlps_hip_loopback shard (1, 4) appends and projects on the rows it owns; shard=(0, 1), a group of one,
  gives the rank of the plain problem."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
G_RANGE, G_RANGE_2 = (-2.0, 2.0), (1.0, -1.5)
T = 4
# all-reduces of an entry ("Several processes"): the projection's one; an append's agreement ahead of the
# product and its sums
PROJECT_ALLREDUCES, APPEND_ALLREDUCES = 1, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _matrix(name):
    import history_ref as H
    from prealps_amd import gen
    if name == "P":
        rp, ci_, v = gen.poisson3d_csr(10)
        return rp, ci_, v, ((np.arange(1000) // 5) % 8).astype(np.int32), 8, True
    if name == "G":
        rp, ci_, v = gen.poisson3d_csr(10)
        return rp, ci_, gen.graded_values(rp, ci_, v, *G_RANGE), None, 8, True
    A, _ = H.heat_matrix()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), None, H.HEAT_PARTS, False


def _describe(rp, ci_, v, N):
    import scipy.sparse as sp
    A0 = sp.csr_matrix((v, ci_, rp), shape=(N, N))
    return dict(A=A0, absA=abs(A0), n_max=int(np.diff(A0.indptr).max()))


def _worst(pb, X, b, x0):
    import history_ref as H
    c = np.linalg.lstsq(X, x0, rcond=None)[0]      # (enters the bounds by its size only)
    rho, bound = H.galerkin(pb["A"], pb["absA"], pb["n_max"], X, list(range(X.shape[1])), b, x0, c)
    return float((np.abs(rho) / bound).max())


def _same_solve(a, b):
    assert a.iters == b.iters
    assert np.asarray(a.x).tobytes() == np.asarray(b.x).tobytes()
    assert a.res.tobytes() == b.res.tobytes() and a.sys_hist.tobytes() == b.sys_hist.tobytes()
    assert a.sys_res_original.tobytes() == b.sys_res_original.tobytes()


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["LOCAL_RANK"] = "0"
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import history_ref as H
        import prealps_amd as pa
        fails = []

        def gathered(obj):
            box = [None] * world
            dist.all_gather_object(box, obj)
            return box

        def same_on_every_rank(obj, what):
            box = gathered(obj)
            assert all(b == box[0] for b in box), "%s differs between the ranks" % what

        def case(name, fn):
            try:
                fn()
            except Exception as e:
                import traceback
                fails.append("case %s: %s\n%s" % (name, e, traceback.format_exc()))

        def build(name):
            rp, ci_, v, part, P, scale = _matrix(name)
            prob = pa.EcgProblem(rp, ci_, v, P, part, scale=scale, device=0, distributed=True)
            prob.create_block_jacobi()
            N = prob.N
            pb = _describe(rp, ci_, v, N)
            own = prob.owned_rows
            others = np.ones(N, dtype=bool)
            others[own] = False
            pb.update(prob=prob, N=N, own=own, others=others, B=np.random.default_rng(20260407).standard_normal((N, 16)))
            owners = gathered(own)
            assert sorted(np.concatenate(owners).tolist()) == list(range(N))
            pb["owners"] = owners
            return pb

        def assembled(pb, x):
            x = np.asarray(x)
            assert not x[pb["others"]].any(), "a row this rank does not own is not zero"
            return sum(gathered(x))

        # ================================================ P ================================================
        pb = build("P")
        prob, N, own, others, B = pb["prob"], pb["N"], pb["own"], pb["others"], pb["B"]
        assert prob.stat("halo_rows") > 0 and (np.diff(own) != 1).any()
        mine = np.column_stack([prob.solve_system(B[:, j], T, tol=1e-8).x for j in range(5)])      # this rank's rows of x
        X = assembled(pb, mine)

        # (1) Galerkin
        def galerkin():
            prob.enable_history(8)
            try:
                prob.history_append(mine)
                assert prob.stat("hist_columns") == 5 and prob.stat("hist_capacity") == 8 and prob.stat("hist_appends") == 5
                assert prob.stat("hist_bytes") == 8.0 * prob.m * 8
                b = B[:, 5]
                x0, rk, captured = prob.history_project(b)
                assert rk == 5 and prob.stat("hist_last_rank") == 5
                assert not x0[others].any() and x0[own].any()
                X0 = assembled(pb, x0)
                w = _worst(pb, X, b, X0)
                print("rank", rank, "world", world, "Galerkin: worst |rho| / bound = %.3e" % w, flush=True)
                assert w <= 1.0
                assert abs(captured[0] - H.energy_norm(pb["A"], X0) ** 2) <= 1e-9 * captured[0]
                x1, rk1, cap1 = prob.history_project(b)
                assert (rk1, cap1.tobytes(), x1[own].tobytes()) == (rk, captured.tobytes(), x0[own].tobytes())
                same_on_every_rank((rk, captured.tobytes()), "rank or captured")
                xd, rkd, capd = prob.history_project(torch.from_numpy(b).cuda())
                assert rkd == 5 and xd.cpu().numpy().tobytes() == x0.tobytes() and capd.tobytes() == captured.tobytes()
                x3, rk3, _ = prob.history_project(B[:, 5:8])
                assert rk3 == 5 and x3[:, 0].tobytes() == x0.tobytes()
                # device tensors enter the ring with the bits of the host path
                prob.clear_history()
                prob.history_append(torch.from_numpy(np.ascontiguousarray(mine)).cuda())
                xa, rka, capa = prob.history_project(b)
                assert rka == 5 and xa.tobytes() == x0.tobytes() and capa.tobytes() == captured.tobytes()
            finally:
                prob.disable_history()
            assert prob.stat("hist_capacity") == 0 and prob.stat("hist_columns") == 0

        case("Galerkin", galerkin)

        # (2) bits
        def bits(k, stop, variant):
            alg = pa.ORTHODIR if variant == "odir" else pa.ORTHOMIN
            B1 = B[:, :k] if k > 1 else B[:, 0]
            B2 = B[:, 4:4 + k] if k > 1 else B[:, 4]
            B2 = B2 + 0.5 * B1                        # (so that the history holds a part of the answer)
            prob.enable_history(8)
            try:
                plain = prob.solve_system(B1, T, stop=stop, ortho_alg=alg, tol=TOL)
                first = prob.solve_system(B1, T, stop=stop, ortho_alg=alg, tol=TOL, history=True)
                _same_solve(first, plain)
                assert first.history_rank == 0 and prob.stat("hist_columns") == k
                assert first.sys_res0.tobytes() == first.sys_normb.tobytes()
                x0, rk, _ = prob.history_project(B2)
                assert rk == k
                ref = prob.solve_system(B2, T, x0=assembled(pb, x0), stop=stop, ortho_alg=alg, tol=TOL)
                got = prob.solve_system(B2, T, stop=stop, ortho_alg=alg, tol=TOL, history=True)
                _same_solve(got, ref)
                assert got.history_rank == k and prob.stat("hist_columns") == 2 * k
                assert (got.sys_res0 < got.sys_normb).all()
                same_on_every_rank((got.iters, got.history_rank, got.sys_res0.tobytes()), "the history solve")
            finally:
                prob.disable_history()

        for k, stop, variant in ((1, "original", "odir"), (2, "scaled", "odir"), (2, "original", "odir"),
                                 (1, "scaled", "odir"), (1, "original", "omin")):
            case("bits %s" % ((k, stop, variant),), lambda: bits(k, stop, variant))

        if world == 2:
            # (3) a repeated right-hand side
            def repeated():
                b = B[:, 0]
                prob.enable_history(8)
                try:
                    first = prob.solve_system(b, T, tol=TOL, history=True)
                    again = prob.solve_system(b, T, tol=TOL, history=True)
                    print("rank", rank, "repeated: start residual / (tol ||b||) = %.3f, %d iterations"
                          % (again.sys_res0[0] / (TOL * np.linalg.norm(b)), again.iters), flush=True)
                    assert again.history_rank == 1
                    assert again.sys_res0[0] <= 8 * TOL * np.linalg.norm(b)
                    assert again.iters <= 2 and first.iters > 2
                    assert prob.stat("hist_columns") == (1 if again.iters == 0 else 2)
                finally:
                    prob.disable_history()

            case("repeated", repeated)

            # (4) capacity 3, five appends: the last three are kept
            def ring():
                b = B[:, 5]
                prob.enable_history(3)
                try:
                    for j in range(5):
                        prob.history_append(mine[:, j])
                    assert prob.stat("hist_columns") == 3 and prob.stat("hist_appends") == 5
                    xa, ra, _ = prob.history_project(b)
                    assert ra == 3
                    w = _worst(pb, X[:, 2:], b, assembled(pb, xa))
                    print("rank", rank, "ring: worst |rho| / bound = %.3e" % w, flush=True)
                    assert w <= 1.0
                    # more columns than the capacity at once: the last three again
                    prob.clear_history()
                    prob.history_append(mine)
                    assert prob.stat("hist_columns") == 3
                    xc, rc, _ = prob.history_project(b)
                    assert rc == 3 and _worst(pb, X[:, 2:], b, assembled(pb, xc)) <= 1.0
                finally:
                    prob.disable_history()

            case("ring", ring)

            # (7) all-reduces per entry
            def collectives():
                prob.enable_history(8)
                try:
                    def cost(fn):
                        before = prob.stat("allreduces")
                        out = fn()
                        return prob.stat("allreduces") - before, out

                    counts = {}
                    n, _ = cost(lambda: prob.history_append(mine[:, 0]))
                    counts["append K=0 q=1"] = n
                    n, _ = cost(lambda: prob.history_project(B[:, 5]))
                    counts["project K=1 q=1"] = n
                    n, _ = cost(lambda: prob.history_append(mine[:, 1]))
                    counts["append K=1 q=1"] = n
                    prob.history_append(mine[:, 2:5])
                    n, _ = cost(lambda: prob.history_project(B[:, 5:8]))
                    counts["project K=5 q=3"] = n
                    prob.clear_history()
                    prob.history_append(mine[:, :2])
                    n, _ = cost(lambda: prob.history_append(mine[:, 2:5]))
                    counts["append K=2 q=3"] = n
                    b2 = B[:, 6] + 0.5 * B[:, 0]
                    x0, rk, _ = prob.history_project(b2)
                    n_solve, ref = cost(lambda: prob.solve_system(b2, T, x0=assembled(pb, x0), tol=TOL))
                    n_hist, got = cost(lambda: prob.solve_system(b2, T, tol=TOL, history=True))
                    print("rank", rank, "all-reduces", counts, "solve_system(x0=)", n_solve, "history=True", n_hist, flush=True)
                    assert counts["project K=1 q=1"] == counts["project K=5 q=3"] == PROJECT_ALLREDUCES
                    assert counts["append K=0 q=1"] == counts["append K=1 q=1"] == counts["append K=2 q=3"] == APPEND_ALLREDUCES
                    assert rk == 5 and got.iters == ref.iters > 0
                    assert n_hist == PROJECT_ALLREDUCES + n_solve + APPEND_ALLREDUCES
                finally:
                    prob.disable_history()

            case("collectives", collectives)

            # (8) refusals reached together
            def refusals():
                L = prob.L
                own0 = pb["owners"][0]
                prob.enable_history(4)
                try:
                    prob.history_append(mine[:, :3])
                    b = np.ascontiguousarray(B[:, 5])
                    before = prob.history_project(b)
                    bn = b.copy()
                    bn[own0[len(own0) // 2]] = np.nan               # a row only rank 0 owns
                    with pytest.raises(pa.PreAlpsError, match="preAlps_SolutionHistoryProject.*not finite"):
                        prob.history_project(bn)
                    assert prob.stat("hist_columns") == 3
                    with pytest.raises(pa.PreAlpsError, match="preAlps_ECGSolveSystemHistory.*not finite"):
                        prob.solve_system(bn, T, tol=TOL, history=True)
                    assert prob.stat("hist_columns") == 3
                    xn = mine[:, 3].copy()
                    if rank == 0:
                        xn[own0[len(own0) // 2]] = np.nan
                    with pytest.raises(pa.PreAlpsError, match="preAlps_SolutionHistoryAppend.*not finite"):
                        prob.history_append(xn)
                    assert prob.stat("hist_columns") == 3 and prob.stat("hist_appends") == 3
                    # a leading dimension that is wrong on rank 1 alone
                    out, rk = np.zeros(N), C.c_int()
                    ld = N - 1 if rank == 1 else N
                    assert L.preAlps_SolutionHistoryProject(1, b.ctypes.data, ld, out.ctypes.data, N, 0, 0.0, C.byref(rk), None) != 0
                    msg = (L.preAlps_hip_last_error() or b"").decode()
                    assert msg.startswith("preAlps_SolutionHistoryProject:") and ("ldb" in msg if rank == 1 else "another process" in msg), msg
                    assert L.preAlps_SolutionHistoryAppend(1, b.ctypes.data, ld, 0) != 0
                    msg = (L.preAlps_hip_last_error() or b"").decode()
                    assert msg.startswith("preAlps_SolutionHistoryAppend:") and ("ldx" in msg if rank == 1 else "another process" in msg), msg
                    assert prob.stat("hist_columns") == 3 and prob.stat("hist_appends") == 3
                    with pytest.raises(pa.PreAlpsError, match="preAlps_ECGSolveSystemHistory.*ADAPT_BS.*single process"):
                        prob.solve_system(b, T, bs_red=pa.ADAPT_BS, tol=TOL, history=True)
                    # ... and the ranks are together afterwards
                    after = prob.history_project(b)
                    assert (after[1], after[2].tobytes(), after[0].tobytes()) == (before[1], before[2].tobytes(), before[0].tobytes())
                    same_on_every_rank(tuple(prob.stat(key) for key in ("hist_columns", "hist_appends", "hist_projections",
                                                                        "hist_gram_refreshes", "hist_last_rank",
                                                                        "hist_values_epoch")), "the history's counters")
                finally:
                    prob.disable_history()

            case("refusals", refusals)
        prob.close()

        # ================================================ G ================================================
        if world == 2:
            # (5) a values update: the refresh is lazy, and there is exactly one
            def values_update():
                import scipy.sparse as sp
                from prealps_amd import gen
                pg = build("G")
                pr = pg["prob"]
                try:
                    Bg = pg["B"]
                    mine_g = np.column_stack([pr.solve_system(Bg[:, j], T, tol=1e-8).x for j in range(5)])
                    Xg = assembled(pg, mine_g)
                    rp, ci_, v0 = gen.poisson3d_csr(10)
                    v2 = gen.graded_values(rp, ci_, v0, *G_RANGE_2)
                    A2 = sp.csr_matrix((v2, ci_, rp), shape=(pg["N"], pg["N"]))
                    new = dict(A=A2, absA=abs(A2), n_max=pg["n_max"])
                    b = Bg[:, 5]
                    pr.enable_history(8)
                    pr.history_append(mine_g)
                    assert pr.stat("hist_gram_refreshes") == 0 and pr.stat("hist_values_epoch") == pr.stat("op_values_epoch")
                    pr.update_values(v2, precond="refactor")
                    assert pr.stat("hist_values_epoch") < pr.stat("op_values_epoch")        # lazy: nothing has happened yet
                    x0, rk, _ = pr.history_project(b)
                    assert rk == 5 and pr.stat("hist_gram_refreshes") == 1
                    assert pr.stat("hist_values_epoch") == pr.stat("op_values_epoch")
                    X0 = assembled(pg, x0)
                    w_new, w_old = _worst(new, Xg, b, X0), _worst(pg, Xg, b, X0)
                    print("rank", rank, "values update: worst |rho| / bound against the new matrix %.3e, the old one %.3e"
                          % (w_new, w_old), flush=True)
                    assert w_new <= 1.0 and w_old > 100.0
                    pr.history_project(b)
                    pr.history_append(mine_g[:, 0])
                    assert pr.stat("hist_gram_refreshes") == 1
                finally:
                    pr.disable_history()
                    pr.close()

            case("values update", values_update)

        # ================================================ H ================================================
        # (6) the heat sequence
        def heat():
            ref = H.heat_reference()
            ph = build("H")
            pr = ph["prob"]
            try:
                pr.enable_history(8)
                u = np.zeros(ph["N"])
                iters, cold = [], []
                for n in range(1, H.HEAT_STEPS + 1):
                    b = H.heat_rhs(u, n)
                    if 8 <= n <= 15:
                        cold.append(pr.solve_system(b, H.HEAT_T, stop="scaled", tol=H.HEAT_TOL).iters)
                    r = pr.solve_system(b, H.HEAT_T, stop="scaled", tol=H.HEAT_TOL, history=True)
                    iters.append(r.iters)
                    u = assembled(ph, r.x)
                print("rank", rank, "world", world, "heat: iterations per step with history %s (restatement %s), cold over "
                      "steps 8..15 %s" % (iters, ref["hist"], cold), flush=True)
                for n, (a, e) in enumerate(zip(iters, ref["hist"]), 1):
                    assert abs(a - e) <= 1, (n, a, e)
                assert sum(iters[7:15]) <= 0.5 * sum(cold), (iters, cold)
                assert pr.stat("hist_columns") == 8 and pr.stat("hist_projections") == H.HEAT_STEPS
            finally:
                pr.disable_history()
                pr.close()

        case("heat", heat)

        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok" if not fails else "fail: " + "\n".join(fails)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc())))


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_sharing_one_gpu_keep_a_solution_history(world):
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
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import history_ref as H
        import prealps_amd as pa
        rp, ci_, v, part, P, scale = _matrix("P")
        N = 1000
        pb = _describe(rp, ci_, v, N)
        B = np.random.default_rng(20260407).standard_normal((N, 16))
        b = np.ascontiguousarray(B[:, 5])
        ranks = {}
        for shard in (None, (0, 1)):       # (the shards last: the loopback hooks stay installed in the process)
            prob = pa.EcgProblem(rp, ci_, v, P, part, scale=scale, device=0, shard=shard)
            prob.create_block_jacobi()
            X = np.column_stack([prob.solve_system(B[:, j], T, tol=1e-8).x for j in range(5)])
            prob.enable_history(8)
            prob.history_append(X)
            x0, rk, captured = prob.history_project(b)
            assert prob.stat("hist_bytes") == 8.0 * N * 8
            w = _worst(pb, X, b, x0)
            print("shard", shard, "rank", rk, "worst |rho| / bound = %.3e" % w, flush=True)
            assert w <= 1.0
            ranks[shard] = rk
            got = prob.solve_system(b, T, tol=TOL, history=True)
            assert got.history_rank == rk and prob.stat("hist_columns") == 6
            prob.close()
        assert ranks[(0, 1)] == ranks[None] == 5
        # rank 1 of 4 rehearsed in one process, its collectives empty: it solves with A0[own][:, own]
        prob = pa.EcgProblem(rp, ci_, v, P, part, scale=scale, device=0, shard=(1, 4))
        prob.create_block_jacobi()
        own = prob.owned_rows
        others = np.ones(N, dtype=bool)
        others[own] = False
        assert prob.m == len(own) == N // 4
        Aoo = pb["A"][own][:, own].tocsr()
        sub = dict(A=Aoo, absA=abs(Aoo), n_max=int(np.diff(Aoo.indptr).max()))
        # (t = 2: the shard owns parts 2 and 3 of 8, and with nothing reduced the columns p % t of a block must all be
        # its own -- at t = 4 two of them would be empty and P^T A P singular)
        ts_ = 2
        X = np.column_stack([prob.solve_system(B[:, j], ts_, tol=1e-8).x for j in range(5)])
        assert np.isfinite(X).all() and X[own].any() and not X[others].any()
        prob.enable_history(8)
        prob.history_append(X)
        assert prob.stat("hist_columns") == 5 and prob.stat("hist_bytes") == 8.0 * prob.m * 8
        sentinel = -12345.678
        out, rk, cap = np.full(N, sentinel), C.c_int(), np.zeros(1)
        from prealps_amd.lib import check
        check(prob.L.preAlps_SolutionHistoryProject(1, b.ctypes.data, N, out.ctypes.data, N, 0, 0.0, C.byref(rk),
                                                    cap.ctypes.data_as(C.POINTER(C.c_double))), "preAlps_SolutionHistoryProject")
        assert (out[others] == sentinel).all(), "a row this shard does not own was written"
        x0, rk2, _ = prob.history_project(b)
        assert rk.value == rk2 == 5 and x0[own].tobytes() == out[own].tobytes() and not x0[others].any()
        c = np.linalg.lstsq(X[own], x0[own], rcond=None)[0]
        rho, bound = H.galerkin(sub["A"], sub["absA"], sub["n_max"], X[own], list(range(5)), b[own], x0[own], c)
        w = float((np.abs(rho) / bound).max())
        print("shard (1, 4): worst |rho| / bound = %.3e" % w, flush=True)
        assert w <= 1.0
        # an x with other rows filled in is read at the owned rows alone
        Xf = X.copy()
        Xf[others] = np.nan
        prob.clear_history()
        prob.history_append(Xf)
        assert prob.history_project(b)[0].tobytes() == x0.tobytes()
        run = prob.solve_system(b, ts_, tol=TOL, history=True)
        assert run.history_rank == 5 and np.isfinite(run.x).all() and not run.x[others].any()
        prob.close()
        q.put("ok")
    except Exception as e:  # pragma: no cover
        import traceback
        q.put("fail: %s\n%s" % (e, traceback.format_exc()))


def test_loopback_shards_keep_a_solution_history_in_one_process():
    """EcgProblem(..., shard=(1, 4)) appends and projects on the rows it owns and writes no other; the projection is
    the Galerkin projection of the matrix the shard solves with, A0[own][:, own]; shard=(0, 1), a group of one, keeps
    the rank of the plain problem (bits are not asked for: g is summed in another row order)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_process_worker, args=(q,))
    p.start()
    res = q.get(timeout=240)
    p.join(timeout=60)
    assert res == "ok", res
