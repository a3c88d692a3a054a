"""Two-level block Jacobi on the GPU: M^-1 = B^-1 + Z E^-1 Z^T (preAlps_BlockJacobiSetCoarseSpace, coarse.hip).
The references are NumPy in fp64: Z, E and its inverse formed from local_csr(), and a restatement of the ECG Orthodir
iteration with M^-1 as a callable.  Iteration counts of the solve test (elasticity 12x10x10, 150 parts, t = 4,
translations, tol 1e-5) are printed by the test and recorded in DESIGN.md section 4j."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = 1e-5


# ---- problems (the operator is process-global in the library: one at a time) ---------------------------------
def _random_spd(n, density, seed):
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=rng, format="csr")
    A = M + M.T
    A = sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0))
    A.sort_indices()
    return A


def _matrix(name):
    """rowptr, colind, val, parts, partition vector, unknowns per node."""
    from prealps_amd import gen
    if name == "poisson5":
        rp, ci, v = gen.poisson3d_csr(12)
        return rp, ci, v, 5, None, 1
    if name == "poisson16":
        rp, ci, v = gen.poisson3d_csr(16)
        return rp, ci, v, 2, None, 1
    if name == "poisson_rows":                     # every row a part of its own: 1728 parts, more than the cap holds
        rp, ci, v = gen.poisson3d_csr(12)
        return rp, ci, v, 1728, None, 1
    if name == "elasticity_cut":
        rp, ci, v = gen.elasticity3d_csr(7)
        return rp, ci, v, 8, None, 3
    if name == "elasticity12":
        nn = (12, 10, 10)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, P = gen.box_partition_nodes(nn, (2, 2, 2))
        return rp, ci, v, P, part, 3
    A = _random_spd(1500, 0.004, 11)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, 7, None, 1


_open = {}


def _problem(name):
    import prealps_amd as pa
    if name in _open:
        return _open[name]
    for other in list(_open):
        _open.pop(other)["prob"].close()
    rp, ci, v, P, part, dofs = _matrix(name)
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    prob.create_block_jacobi()
    _open[name] = dict(prob=prob, dofs=dofs, mat=(rp, ci, v, P, part), cache={})
    return _open[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for name in list(_open):
        _open.pop(name)["prob"].close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _vectors(pb, k):
    """k vectors in the caller's order: the translations where they exist, random columns beside them."""
    from prealps_amd.nearkernel import translations
    N, dofs = pb["prob"].N, pb["dofs"]
    T = translations(N, dofs)
    if k <= dofs:
        return np.asfortranarray(T[:, :k])
    extra = np.random.default_rng(100 + k).standard_normal((N, k - dofs))
    return np.asfortranarray(np.hstack([T, extra]))


def _aggregates(prob, mode):
    if mode == "one":
        return np.arange(prob.nparts, dtype=np.int32)
    return (np.arange(prob.nparts) // (3 if prob.nparts > 6 else 2)).astype(np.int32)


def _numpy_coarse(prob, V, aggr):
    """A' (the operator's own matrix), Z, E and inv(E) in fp64 from local_csr(), the permutation and the scaling."""
    lrp, lci, lv = prob.local_csr()
    A = sp.csr_matrix((lv, lci, lrp), shape=(prob.m, prob.M))
    d = prob.scaling
    Vp = (V / d[:, None])[prob.perm] if d is not None else V[prob.perm]
    m, k = Vp.shape
    g = np.repeat(np.asarray(aggr), np.diff(prob.rowpos))
    rows = np.repeat(np.arange(m), k)
    cols = (g[:, None] * k + np.arange(k)[None, :]).ravel()
    Z = sp.csr_matrix((Vp.ravel(), (rows, cols)), shape=(m, (int(np.max(aggr)) + 1) * k))
    E = (Z.T @ A @ Z).toarray()
    return A, Z, E, np.linalg.inv(E)


# ---- the apply --------------------------------------------------------------------------------------------------
_APPLY = [("poisson5", 1, "one"), ("poisson5", 3, "several"), ("elasticity_cut", 3, "one"), ("elasticity_cut", 6, "several"),
          ("elasticity12", 3, "one"), ("elasticity12", 1, "several"), ("random7", 3, "one"), ("random7", 6, "several")]


def _check_apply(pb, k, mode, strides=(4, 8, 16)):
    prob = pb["prob"]
    prob.clear_coarse_space()
    V, aggr = _vectors(pb, k), (None if mode == "default" else _aggregates(prob, mode))
    rng = np.random.default_rng(7 * k + prob.nparts)
    W = {t: rng.standard_normal((prob.m, t if t < 16 else 13)) for t in strides}      # 13 live columns at stride 16
    plain = {t: prob.block_jacobi_apply(W[t], t) for t in strides}
    prob.set_coarse_space(V, aggr)
    if aggr is None:                                       # the library's own choice
        aggr = prob.coarse_aggregates()
        assert len(np.unique(aggr)) == aggr.max() + 1      # numbered without gaps
    A, Z, E, Einv = _numpy_coarse(prob, V, aggr)
    nc = E.shape[0]
    assert prob.stat("bj_coarse_dofs") == nc and prob.stat("bj_coarse_vectors") == k
    assert prob.stat("bj_coarse_aggregates") == aggr.max() + 1 and prob.stat("bj_coarse_bytes") > 8 * nc * nc
    assert prob.stat("bj_coarse_chunks") >= prob.nparts
    assert nc <= prob.stat("bj_coarse_max_dofs")
    cond = np.linalg.cond(E)
    bound = 100 * nc * EPS * cond
    print("%d coarse unknowns, cond_2(E) = %.3e, bound %.3e" % (nc, cond, bound))
    n0 = prob.stat("bj_coarse_applies")
    for t in strides:
        got = prob.block_jacobi_apply(W[t], t)
        coarse = Z @ (Einv @ (Z.T @ W[t]))
        err = np.linalg.norm(got - (plain[t] + coarse)) / np.linalg.norm(coarse)
        print("stride %2d: relative error of the coarse term %.3e" % (t, err))
        assert err <= bound
        assert _same_bits(got, prob.block_jacobi_apply(W[t], t))                     # two applies agree in bits
    assert prob.stat("bj_coarse_applies") == n0 + 2 * len(strides)
    # projection: Z Einv Z^T (A' Z w) = Z w
    t = 4
    w = rng.standard_normal((nc, t))
    Zw = Z @ w
    AZw = prob.block_operator(Zw, t)
    got = prob.block_jacobi_apply(AZw, t) - _plain_apply_of(prob, V, aggr, AZw, t)
    err = np.linalg.norm(got - Zw) / np.linalg.norm(Zw)
    print("projection: %.3e" % err)
    assert err <= bound
    # symmetry of M^-1
    U, Wm = rng.standard_normal((prob.m, t)), rng.standard_normal((prob.m, t))
    a = np.sum(U * prob.block_jacobi_apply(Wm, t))
    b = np.sum(prob.block_jacobi_apply(U, t) * Wm)
    print("symmetry: <U, M^-1 W> = %.15e, <M^-1 U, W> = %.15e, relative difference %.3e" % (a, b, abs(a - b) / max(abs(a), abs(b))))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    prob.clear_coarse_space()


def _plain_apply_of(prob, V, aggr, X, t):
    """B^-1 X with the coarse space taken off and put back (the same vectors and aggregates)."""
    prob.clear_coarse_space()
    out = prob.block_jacobi_apply(X, t)
    prob.set_coarse_space(V, aggr)
    return out


@pytest.mark.parametrize("name,k,mode", _APPLY)
def test_apply_is_block_jacobi_plus_the_coarse_term(name, k, mode):
    _check_apply(_problem(name), k, mode)


@pytest.mark.parametrize("k,mode", [(1, "one"), (3, "several")])
def test_apply_on_top_of_sparse_factors(monkeypatch, k, mode):
    """Nested-dissection blocks (PREALPS_BJ_ND=2 as test_gpu_distributed sets it), Poisson 16^3 in two parts of 2048
    rows: the apply test above with its strides, every aggregate summed from two chunks (one aggregate per part) or
    four (both parts in one aggregate, three vectors)."""
    for other in list(_open):
        _open.pop(other)["prob"].close()
    monkeypatch.setenv("PREALPS_BJ_ND", "2")
    monkeypatch.setenv("PREALPS_BJ_ND_ROWS", "512")
    monkeypatch.setenv("PREALPS_ND_LEAF", "32")
    pb = _problem("poisson16")
    try:
        assert pb["prob"].stat("bj_nd_blocks") == 2
        _check_apply(pb, k, mode)
    finally:
        _open.pop("poisson16")["prob"].close()


def test_default_aggregates_from_the_partitioner_when_the_parts_exceed_the_cap():
    """1728 one-row parts, one vector: more unknowns than the cap, so the aggregates come from
    preAlps_hip_partition_kway on the quotient graph of the parts; then the apply test on what the library chose."""
    pb = _problem("poisson_rows")
    prob = pb["prob"]
    cap = int(prob.stat("bj_coarse_max_dofs"))
    assert prob.nparts > cap
    try:
        _check_apply(pb, 1, "default", strides=(4,))
        prob.set_coarse_space(_vectors(pb, 1))
        agg = prob.coarse_aggregates()
        naggr = int(prob.stat("bj_coarse_aggregates"))
        assert naggr == agg.max() + 1 and cap // 2 < naggr <= cap
        print("%d parts in %d aggregates, %d parts in the largest" % (prob.nparts, naggr, np.bincount(agg).max()))
        assert np.bincount(agg).min() >= 1                                          # none empty
    finally:
        _open.pop("poisson_rows")["prob"].close()


def test_refused_without_a_preconditioner_and_the_accessor_without_a_coarse_space():
    import prealps_amd as pa
    for other in list(_open):
        _open.pop(other)["prob"].close()
    rp, ci, v, P, part, dofs = _matrix("poisson5")
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    try:
        V = np.ones((prob.N, 1), order="F")
        rc = prob.L.preAlps_BlockJacobiSetCoarseSpace(1, V.ctypes.data_as(C.POINTER(C.c_double)), prob.N, None, 0)
        msg = prob.L.preAlps_hip_last_error().decode()
        assert rc != 0 and "preconditioner not created" in msg and "preAlps_BlockJacobiSetCoarseSpace" in msg
        prob.create_block_jacobi()
        with pytest.raises(pa.PreAlpsError, match="no coarse space"):
            prob.coarse_aggregates()
        prob.set_coarse_space(V)
        assert np.array_equal(prob.coarse_aggregates(), np.arange(P))
    finally:
        prob.close()


# ---- captured iteration segments --------------------------------------------------------------------------------
def test_a_solver_that_replays_graphs_follows_set_and_clear():
    """preAlps_hip_graphs(1): a solver captures the two halves of an iteration on their second pass and replays them.
    A coarse space set or cleared between two preAlps_ECGAdvance calls changes the launches of the apply and frees
    device arrays the graphs point to, so the solver must capture anew.  The same sequence without graphs is the
    reference; a stale graph would apply the other preconditioner, an O(1) difference in the residual."""
    import prealps_amd as pa
    from prealps_amd.lib import check
    pb = _problem("elasticity12")
    prob = pb["prob"]
    L = prob.L
    pd = C.POINTER(C.c_double)
    b = np.random.default_rng(4).standard_normal(prob.m)
    V = _vectors(pb, 3)

    def run(graphs):
        prob.clear_coarse_space()
        L.preAlps_hip_graphs(graphs)
        try:
            e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, 1e-12, 1000)
            rci, rhs, sol = C.c_int(0), np.ascontiguousarray(b), np.zeros(prob.m)
            check(L.preAlps_hip_prepare_operator(4), "prepare")
            check(L.preAlps_ECGInitialize(C.byref(e), rhs.ctypes.data_as(pd), C.byref(rci)), "initialize")
            res, caps = [], []
            for step in ("plain", "coarse", "coarse2", "plain"):
                if step == "coarse":
                    prob.set_coarse_space(V)
                elif step == "coarse2":
                    prob.set_coarse_space(V, _aggregates(prob, "several"))       # a replacement: new arrays
                else:
                    prob.clear_coarse_space()
                r, it, lr = C.c_int(), C.c_int(), C.c_double()
                cap0 = prob.stat("ecg_graph_captures")
                check(L.preAlps_ECGAdvance(C.byref(e), rhs.ctypes.data_as(pd), C.byref(rci), 8, C.byref(r), C.byref(it),
                                           C.byref(lr)), "advance")
                res.append(e.res)
                caps.append(prob.stat("ecg_graph_captures") - cap0)
            check(L.preAlps_ECGFinalize(C.byref(e), sol.ctypes.data_as(pd)), "finalize")
            return np.array(res), sol, caps
        finally:
            L.preAlps_hip_graphs(-1)                      # follow PREALPS_ECG_GRAPH again
            prob.clear_coarse_space()

    ref, xref, caps0 = run(0)
    rep0 = prob.stat("ecg_graph_replays")
    got, x, caps = run(1)
    # the graphs were in use, and every change of the apply made the solver capture anew: a (half, phase) segment is
    # captured on its second pass, and the 8 iterations of a call pass two of the six phases twice
    assert caps0 == [0, 0, 0, 0] and prob.stat("ecg_graph_replays") > rep0
    print("segments captured per call:", caps)
    assert all(c > 0 for c in caps)
    print("residual norms after each 8 iterations (plain, coarse, replaced, plain): launches %s, graphs %s" % (ref, got))
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, ref, rtol=1e-6)
    np.testing.assert_allclose(x, xref, rtol=1e-6, atol=1e-9 * np.abs(xref).max())


# ---- off means off ----------------------------------------------------------------------------------------------
def test_off_means_off_and_the_gram_by_product_stays_away_while_attached():
    import prealps_amd as pa
    from prealps_amd.lib import check
    pb = _problem("elasticity12")
    prob = pb["prob"]
    prob.clear_coarse_space()
    rng = np.random.default_rng(3)
    W, b = rng.standard_normal((prob.m, 4)), rng.standard_normal(prob.m)
    apply0 = prob.block_jacobi_apply(W, 4)
    g0 = prob.stat("bj_gram_applies")
    sol0 = prob.solve(b, 4)
    g1 = prob.stat("bj_gram_applies")
    assert g1 > g0                                        # plain block Jacobi: the block solve leaves the Gram block
    prob.set_coarse_space(_vectors(pb, 3))
    assert prob.stat("bj_coarse_dofs") == 450
    sol1 = prob.solve(b, 4)
    assert prob.stat("bj_gram_applies") == g1 and sol1.iters < sol0.iters
    # a solver initialised before the attach, driven through the C loop
    prob.clear_coarse_space()
    L = prob.L
    e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, TOL, 1000)
    rci, rhs, sol = C.c_int(0), np.ascontiguousarray(b), np.zeros(prob.m)
    pd = C.POINTER(C.c_double)
    check(L.preAlps_hip_prepare_operator(4), "prepare")
    check(L.preAlps_ECGInitialize(C.byref(e), rhs.ctypes.data_as(pd), C.byref(rci)), "initialize")
    prob.set_coarse_space(_vectors(pb, 3))
    g2 = prob.stat("bj_gram_applies")
    restarts, last_it, last_res = C.c_int(), C.c_int(), C.c_double()
    check(L.preAlps_ECGAdvance(C.byref(e), rhs.ctypes.data_as(pd), C.byref(rci), 12, C.byref(restarts), C.byref(last_it),
                                  C.byref(last_res)), "advance")
    assert prob.stat("bj_gram_applies") == g2
    assert np.isfinite(e.res) and e.res < e.normb
    check(L.preAlps_ECGFinalize(C.byref(e), sol.ctypes.data_as(pd)), "finalize")
    # off again: the bits of before
    prob.clear_coarse_space()
    for key in ("bj_coarse_dofs", "bj_coarse_bytes", "bj_coarse_builds", "bj_coarse_applies", "bj_coarse_einv_address"):
        assert prob.stat(key) == 0
    assert _same_bits(prob.block_jacobi_apply(W, 4), apply0)
    g3 = prob.stat("bj_gram_applies")
    sol2 = prob.solve(b, 4)
    assert sol2.iters == sol0.iters and _same_bits(sol2.x, sol0.x) and _same_bits(sol2.res, sol0.res)
    assert prob.stat("bj_gram_applies") > g3


# ---- the solve ---------------------------------------------------------------------------------------------------
def _split(V, rowpos, s):
    N, k = V.shape
    out = np.zeros((N, k * s))
    for p in range(len(rowpos) - 1):
        for j in range(k):
            out[rowpos[p]:rowpos[p + 1], j * s + p % s] = V[rowpos[p]:rowpos[p + 1], j]
    return out


def _restate(A, rowpos, precond, B, s, tol=TOL, max_iter=600):
    """The ECG Orthodir iteration on R0 = the split of the k columns of B into s columns each, with M^-1 = precond.
    Returns the per-system residual history (iterations x k) and the k solutions."""
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
    return np.array(hist), X.reshape(N, k, s).sum(axis=2)


def test_solve_follows_the_restatement_and_needs_fewer_iterations():
    pb = _problem("elasticity12")
    prob = pb["prob"]
    prob.clear_coarse_space()
    rng = np.random.default_rng(20261019)
    Bi = rng.standard_normal((prob.m, 2))                  # internal space: solve / solve_multi
    plain = prob.solve_multi(Bi[:, :1], 4, tol=TOL)
    plain2 = prob.solve_multi(Bi, 4, tol=TOL)
    V = _vectors(pb, 3)
    aggr = _aggregates(prob, "one")
    prob.set_coarse_space(V)                               # default aggregates: one per part (450 <= cap)
    assert prob.stat("bj_coarse_aggregates") == 150
    A, Z, E, Einv = _numpy_coarse(prob, V, aggr)
    rowpos = np.asarray(prob.rowpos, dtype=np.int64)
    inv = [np.linalg.inv(A[r0:r1, r0:r1].toarray()) for r0, r1 in zip(rowpos[:-1], rowpos[1:])]

    def precond(X):
        Y = np.empty_like(X)
        for p in range(len(inv)):
            Y[rowpos[p]:rowpos[p + 1]] = inv[p] @ X[rowpos[p]:rowpos[p + 1]]
        return Y + Z @ (Einv @ (Z.T @ X))

    got = prob.solve_multi(Bi[:, :1], 4, tol=TOL)
    hist, xref = _restate(A, rowpos, precond, Bi[:, :1], 4)
    print("iterations to %g: block Jacobi %d, with the coarse space %d (restatement %d)" % (TOL, plain.iters, got.iters, len(hist)))
    assert abs(got.iters - len(hist)) <= 1
    np.testing.assert_allclose(got.sys_hist[:8, 0], hist[:8, 0], rtol=1e-8)
    assert got.iters < plain.iters
    same = prob.solve(Bi[:, 0], 4, tol=TOL)                # the driver loop of one system: the same apply
    assert abs(same.iters - len(hist)) <= 1 and same.iters < plain.iters
    # the caller's own system, stopped on the caller's residual; a fresh residual confirms it
    d = prob.scaling
    b = np.empty(prob.N)
    b[prob.perm] = Bi[:, 0]
    b /= d
    sys_ = prob.solve_system(b, 4, stop="original", tol=TOL)
    res, normb = prob.system_residuals(b, sys_.x)
    print("solve_system: %d iterations, fresh residual %.3e of %.3e" % (sys_.iters, res[0], normb[0]))
    assert res[0] <= TOL * normb[0]
    # two right-hand sides at t = 4
    two = prob.solve_multi(Bi, 4, tol=TOL)
    print("two right-hand sides: block Jacobi %d, with the coarse space %d" % (plain2.iters, two.iters))
    assert (two.sys_res <= TOL * two.sys_normb).all() and two.iters < plain2.iters
    fresh = np.linalg.norm(Bi - A @ two.x, axis=0)
    assert (fresh <= np.sqrt(2.0) * TOL * np.linalg.norm(Bi, axis=0) * (1 + 1e-6)).all()
    prob.clear_coarse_space()


# ---- a values update ---------------------------------------------------------------------------------------------
def _new_values(rp, ci, v):
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    rows = np.repeat(np.arange(N), np.diff(rp))
    return s[rows] * v * s[ci]


def test_the_coarse_space_follows_a_values_update():
    import prealps_amd as pa
    from prealps_amd.lib import check
    for other in list(_open):
        _open.pop(other)["prob"].close()
    rp, ci, v, P, part, dofs = _matrix("elasticity_cut")
    v2 = _new_values(rp, ci, v)
    from prealps_amd.nearkernel import translations
    V = translations(len(rp) - 1, 3)
    aggr = np.arange(P, dtype=np.int32) // 2
    W = np.random.default_rng(5).standard_normal((len(rp) - 1, 4))
    fresh = pa.EcgProblem(rp, ci, v2, P, part, scale=True, device=0)
    try:
        fresh.create_block_jacobi()
        fresh.set_coarse_space(V, aggr)
        want = fresh.block_jacobi_apply(W, 4)
        b = np.random.default_rng(6).standard_normal(fresh.m)
        iters_fresh = fresh.solve(b, 4).iters
    finally:
        fresh.close()
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    try:
        prob.create_block_jacobi(coarse=V)
        assert prob.stat("bj_coarse_aggregates") == P
        prob.set_coarse_space(V, aggr)                      # setting one again replaces it
        assert prob.stat("bj_coarse_aggregates") == 4 and prob.stat("bj_coarse_builds") == 1
        addr = prob.stat("bj_coarse_einv_address")
        before = prob.block_jacobi_apply(W, 4)
        prob.update_values(v2, precond="keep")              # lagged factor and coarse space: still SPD, still converges
        assert _same_bits(prob.block_jacobi_apply(W, 4), before)
        lag = prob.solve(b, 4)
        assert lag.final_res <= TOL * lag.normb
        prob.update_values(v2, precond="refactor")
        assert prob.stat("bj_coarse_builds") == 2 and prob.stat("bj_coarse_einv_address") == addr
        assert _same_bits(prob.block_jacobi_apply(W, 4), want)
        assert prob.solve(b, 4).iters == iters_fresh
        prob.update_values(v, precond="rebuild")            # a new factor: the remembered coarse space is attached again
        assert prob.stat("bj_coarse_builds") == 1 and prob.stat("bj_coarse_aggregates") == 4
        assert _same_bits(prob.block_jacobi_apply(W, 4), before)
        # refusals leave the coarse space that is there
        from prealps_amd.lib import PreAlpsError
        with pytest.raises(PreAlpsError, match="aggregate 1 is empty"):
            prob.set_coarse_space(V, np.array([0, 0, 0, 0, 2, 2, 2, 2]))
        Vd = V.copy()
        Vd[:, 1] = Vd[:, 0]
        with pytest.raises(PreAlpsError, match="aggregate 0, vector 1"):
            prob.set_coarse_space(Vd, aggr)
        cap = int(prob.stat("bj_coarse_max_dofs"))
        with pytest.raises(PreAlpsError, match="the cap is %d" % cap):
            prob.L.preAlps_BlockJacobiSetCoarseSpace.restype = C.c_int
            check(prob.L.preAlps_BlockJacobiSetCoarseSpace(3, V.ctypes.data_as(C.POINTER(C.c_double)), len(rp) - 1,
                                                              aggr.ctypes.data_as(C.POINTER(C.c_int)), cap // 3 + 1), "set")
        assert prob.stat("bj_coarse_aggregates") == 4 and _same_bits(prob.block_jacobi_apply(W, 4), before)
    finally:
        prob.close()
