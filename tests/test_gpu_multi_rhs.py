"""Several right-hand sides in one ECG block iteration (preAlps_ECGInitializeMulti / SolveMulti / FinalizeMulti,
EcgProblem.solve_multi): k systems of s = t / k columns each, a per-system stopping test, a per-system finish.

Problems: P = Poisson 10^3, 8 contiguous parts (blocks of 125 rows, band 100); E = elasticity on 12 x 10 x 10 nodes
with boxes of 2 x 2 x 2 nodes (the problem of test_gpu_solve_first.py).  The checker is a NumPy restatement of the
Orthodir iteration (below) on the library's own scaled and permuted matrix (local_csr) and its rowPos."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

TOL = 1e-5
RTOL_HIST = 1e-8          # Poisson histories against another fp64 implementation


# ---- problems (the operator is process-global in the library: one at a time) ---------------------------------
_open = {}


def _problem(name):
    import prealps_amd as pa
    from prealps_amd import gen
    if name in _open:
        return _open[name]
    for other in list(_open):
        _open.pop(other)["prob"].close()
    if name == "P":
        rp, ci, v = gen.poisson3d_csr(10)
        prob = pa.EcgProblem(rp, ci, v, 8, None, scale=True, device=0)
    else:
        nn = (12, 10, 10)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, nparts = gen.box_partition_nodes(nn, (2, 2, 2))
        prob = pa.EcgProblem(rp, ci, v, nparts, part, scale=True, device=0)
    prob.create_block_jacobi()
    lrp, lci, lv = prob.local_csr()
    A = sp.csr_matrix((lv, lci, lrp), shape=(prob.m, prob.M))
    rowpos = np.asarray(prob.rowpos, dtype=np.int64)
    rng = np.random.default_rng(20260407)
    _open[name] = dict(prob=prob, A=A, rowpos=rowpos, B=rng.standard_normal((prob.m, 16)), cache={})
    return _open[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for name in list(_open):
        _open.pop(name)["prob"].close()


def _split(b, rowpos, t):
    """R0 of one system: the rows of part p in column p % t."""
    B = np.zeros((len(b), t))
    for p in range(len(rowpos) - 1):
        B[rowpos[p]:rowpos[p + 1], p % t] = b[rowpos[p]:rowpos[p + 1]]
    return B


# ---- the NumPy restatement of Orthodir -------------------------------------------------------------------------
def _block_inverses(pb):
    if "inv" not in pb["cache"]:
        A, rowpos = pb["A"], pb["rowpos"]
        pb["cache"]["inv"] = [np.linalg.inv(A[rowpos[p]:rowpos[p + 1], rowpos[p]:rowpos[p + 1]].toarray())
                              for p in range(len(rowpos) - 1)]
    return pb["cache"]["inv"]


def _restate(pb, B, s, tol=TOL, max_iter=500):
    """Orthodir on R0 = the split of the k columns of B into s columns each.  Returns the per-system history
    (iterations x k, absolute), the k solutions and ||b_j||."""
    A, rowpos, inv = pb["A"], pb["rowpos"], _block_inverses(pb)
    N, k = B.shape
    t, nparts = k * s, len(rowpos) - 1

    def precond(X):
        Y = np.empty_like(X)
        for p in range(nparts):
            Y[rowpos[p]:rowpos[p + 1]] = inv[p] @ X[rowpos[p]:rowpos[p + 1]]
        return Y

    R = np.zeros((N, t))
    for p in range(nparts):
        for j in range(k):
            R[rowpos[p]:rowpos[p + 1], j * s + p % s] = B[rowpos[p]:rowpos[p + 1], j]
    nb = np.linalg.norm(B, axis=0)
    X = np.zeros((N, t))
    Pm, Pp, APp = precond(R), np.zeros((N, t)), np.zeros((N, t))
    hist = []
    for _ in range(max_iter):
        AP = A @ Pm
        U = np.linalg.cholesky(Pm.T @ AP).T                  # P^T A P = U^T U
        Pm, AP = np.linalg.solve(U.T, Pm.T).T, np.linalg.solve(U.T, AP.T).T
        alpha = Pm.T @ R
        X += Pm @ alpha
        R -= AP @ alpha
        g = np.sqrt((R ** 2).reshape(N, k, s).sum(axis=(0, 2)))
        hist.append(g)
        if not (g > tol * nb).any():
            break
        Z = precond(AP)
        Z -= np.hstack([Pm, Pp]) @ (np.hstack([AP, APp]).T @ Z)     # beta = [AP | AP_prev]^T Z
        Pp, APp, Pm = Pm, AP, Z
    return np.array(hist), X.reshape(N, k, s).sum(axis=2), nb


def _variants():
    import prealps_amd as pa
    return {"odir": (pa.ORTHODIR, pa.NO_BS_RED), "omin": (pa.ORTHOMIN, pa.NO_BS_RED),
            "odir-adapt": (pa.ORTHODIR, pa.ADAPT_BS), "omin-adapt": (pa.ORTHOMIN, pa.ADAPT_BS)}


# ---- control on the single-system solve ------------------------------------------------------------------------
def test_restatement_reproduces_the_single_system_solve():
    """k = 1, s = 4 on P: the restatement gives prob.solve(rhs, 4)'s history to 1e-8 with the same count."""
    pb = _problem("P")
    prob = pb["prob"]
    rhs = prob.reference_rhs()
    got = prob.solve(rhs, 4, tol=TOL)
    hist, x, nb = _restate(pb, rhs[:, None], 4)
    assert len(hist) == got.iters == len(got.res)
    np.testing.assert_allclose(got.res, hist[:, 0], rtol=RTOL_HIST)


# ---- 3. general right-hand sides against the restatement -------------------------------------------------------
@pytest.mark.parametrize("k,s", [(2, 1), (4, 1), (2, 2), (3, 1), (8, 1), (4, 2), (3, 4), (16, 1)])
def test_general_right_hand_sides_follow_the_restatement(k, s):
    """P, seeded standard_normal B, Orthodir: t = 2, 4, 4, 3 (stride 4), 8, 8, 12 (stride 16), 16."""
    pb = _problem("P")
    B = pb["B"][:, :k]
    got = pb["prob"].solve_multi(B, k * s, tol=TOL)
    hist, x, nb = _restate(pb, B, s)
    assert got.sys_hist.shape == (got.iters, k) and got.x.shape == (pb["prob"].m, k)
    assert got.iters == len(hist)
    np.testing.assert_allclose(got.sys_normb, nb, rtol=1e-14)
    np.testing.assert_allclose(got.sys_hist, hist, rtol=RTOL_HIST)
    np.testing.assert_array_equal(got.sys_res, got.sys_hist[-1])
    assert got.normb == pytest.approx(np.linalg.norm(B), rel=1e-14)


# ---- 4. every variant solves every system ----------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["odir", "omin", "odir-adapt", "omin-adapt"])
@pytest.mark.parametrize("k,s", [(4, 1), (2, 2), (4, 2)])
@pytest.mark.parametrize("name", ["P", "E"])
def test_every_variant_solves_every_system(name, k, s, variant):
    """At the stop every system is under its own threshold; the true residual of system j obeys the sqrt(s) bound
    (with the factor 4.0 and the 1e-12 of test_gpu_configs.py for true against recurrence residual); and the
    per-system sums add up to the Frobenius norm the scalar history records."""
    pb = _problem(name)
    alg, red = _variants()[variant]
    B = pb["B"][:, :k]
    got = pb["prob"].solve_multi(B, k * s, ortho_alg=alg, bs_red=red, tol=TOL, max_iter=1000)
    assert 0 < got.iters < 1000 and len(got.res) == got.iters == len(got.sys_hist)
    true = np.linalg.norm(B - pb["A"] @ got.x, axis=0)
    print(name, k, s, variant, "iters", got.iters, "sys_res/normb", got.sys_res / got.sys_normb,
          "true/sys_res", true / got.sys_res)
    assert (got.sys_res <= TOL * got.sys_normb).all(), (got.sys_res, got.sys_normb)
    assert (true <= 4.0 * np.sqrt(s) * got.sys_res + 1e-12).all(), (true, got.sys_res)
    np.testing.assert_allclose((got.sys_hist ** 2).sum(axis=1), got.res ** 2, rtol=1e-13)


# ---- 5. the caller's own loop ----------------------------------------------------------------------------------
def test_the_callers_loop_gives_the_librarys_result():
    """(k, s) = (2, 2) on P through InitializeMulti, the RCI calls in the order of the reference driver,
    preAlps_ECGSystemResiduals after each stopping test and FinalizeMulti."""
    import prealps_amd as pa
    from prealps_amd.lib import check
    pb = _problem("P")
    prob, L = pb["prob"], pb["prob"].L
    k, s, m = 2, 2, pb["prob"].m
    B = np.asfortranarray(pb["B"][:, :k])
    want = prob.solve_multi(B, k * s, tol=TOL)
    pd = C.POINTER(C.c_double)
    e = prob.new_ecg(k * s, pa.ORTHODIR, pa.NO_BS_RED, TOL, 1000)
    rci, stop = C.c_int(0), C.c_int(0)
    check(L.preAlps_ECGInitializeMulti(C.byref(e), k, B.ctypes.data_as(pd), m, C.byref(rci)), "init")
    nb = np.zeros(k)
    check(L.preAlps_ECGSystemResiduals(C.byref(e), None, nb.ctypes.data_as(pd)), "normb")
    check(L.preAlps_BlockJacobiApply(e.R, e.P), "apply")
    check(L.preAlps_BlockOperator(e.P, e.AP), "product")
    hist = []
    while len(hist) < 1000:
        check(L.preAlps_ECGIterate(C.byref(e), C.byref(rci)), "iterate")
        if rci.value == 0:
            check(L.preAlps_BlockOperator(e.P, e.AP), "product")
        else:
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
    assert iters == want.iters == len(hist)
    np.testing.assert_array_equal(nb, want.sys_normb)
    np.testing.assert_allclose(np.array(hist), want.sys_hist, rtol=1e-8)
    np.testing.assert_allclose(x, want.x, rtol=1e-8, atol=1e-8 * np.abs(want.x).max())


# ---- 1. one system is today's solve ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["odir", "omin"])
@pytest.mark.parametrize("t", [1, 2, 4, 8])
def test_one_system_is_the_single_system_solve(t, variant):
    pb = _problem("E")
    prob = pb["prob"]
    alg, red = _variants()[variant]
    b = prob.reference_rhs()
    one = prob.solve(b, t, ortho_alg=alg, bs_red=red, tol=TOL)
    got = prob.solve_multi(b[:, None], t, ortho_alg=alg, bs_red=red, tol=TOL)
    assert got.iters == one.iters and got.x.shape == (prob.m, 1)
    assert got.res.tobytes() == one.res.tobytes() and got.bs.tobytes() == one.bs.tobytes()
    assert np.ascontiguousarray(got.x[:, 0]).tobytes() == one.x.tobytes()
    assert got.normb == one.normb and got.sys_normb[0] == one.normb
    np.testing.assert_array_equal(got.sys_hist[:, 0], one.res)


# ---- 2. the split as right-hand sides --------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["odir", "omin", "odir-adapt", "omin-adapt"])
@pytest.mark.parametrize("t", [4, 8])
def test_the_split_as_right_hand_sides_runs_the_same_launches(t, variant):
    """B = split(b) with k = t, s = 1 starts from the R0 of the single-system solve: eight iterations of both give
    the same bytes of the scalar history, and the solutions of the t systems add up to the single one."""
    pb = _problem("E")
    prob = pb["prob"]
    alg, red = _variants()[variant]
    b = prob.reference_rhs()
    one = prob.solve(b, t, ortho_alg=alg, bs_red=red, tol=TOL, max_iter=8)
    got = prob.solve_multi(_split(b, pb["rowpos"], t), t, ortho_alg=alg, bs_red=red, tol=TOL, max_iter=8)
    assert one.iters == 8 and got.iters == 8
    assert got.res.tobytes() == one.res.tobytes() and got.bs.tobytes() == one.bs.tobytes()
    np.testing.assert_allclose(got.x.sum(axis=1), one.x, rtol=1e-12, atol=1e-12 * np.abs(one.x).max())


# ---- 6. refusals ------------------------------------------------------------------------------------------------
def _refused(L, rc, entry, *reasons):
    assert rc != 0
    msg = L.preAlps_hip_last_error().decode()
    assert entry in msg, msg
    for r in reasons:
        assert r in msg, msg


def test_refusals_name_the_entry_point_and_the_reason():
    import prealps_amd as pa
    import prealps_amd.lib as pl
    from prealps_amd.lib import check
    pb = _problem("P")
    prob, L, m = pb["prob"], pb["prob"].L, pb["prob"].m
    pd = C.POINTER(C.c_double)
    B = np.asfortranarray(pb["B"][:, :4])
    pB = B.ctypes.data_as(pd)
    x = np.zeros((m, 4), order="F")
    px = x.ctypes.data_as(pd)
    rci = C.c_int(0)

    def init(t, k, rhs=pB, ld=m, alg=pa.ORTHODIR):
        e = prob.new_ecg(t, alg, pa.NO_BS_RED, TOL, 100)
        return e, L.preAlps_ECGInitializeMulti(C.byref(e), k, rhs, ld, C.byref(rci))

    entry = "preAlps_ECGInitializeMulti"
    _refused(L, init(4, 0)[1], entry, "nrhs = 0")
    _refused(L, init(4, -2)[1], entry, "nrhs = -2")
    _refused(L, init(4, 3)[1], entry, "not a multiple of nrhs = 3")
    _refused(L, init(16, 1)[1], entry, "size: 8", "enlarging factor per system: 16")
    _refused(L, init(4, 2, ld=m - 1)[1], entry, "ldrhs = %d" % (m - 1))
    Z = B.copy(order="F")
    Z[:, 2] = 0.0
    _refused(L, init(4, 4, rhs=Z.ctypes.data_as(pd))[1], entry, "right-hand side 2 has norm zero")
    _refused(L, init(4, 1, rhs=np.zeros(m).ctypes.data_as(pd))[1], entry, "right-hand side 0 has norm zero")
    _refused(L, init(4, 2, alg=pa.ORTHODIR_FUSED)[1], entry, "ORTHODIR_FUSED")
    try:
        check(L.preAlps_hip_set_world(0, 2), "set_world")
        _refused(L, init(4, 2)[1], entry, "single process", "2 processes")
    finally:
        check(L.preAlps_hip_set_world(0, 1), "set_world")
    try:
        check(L.preAlps_hip_loopback(0, 1), "loopback")
        _refused(L, init(4, 2)[1], entry, "single process", "preAlps_hip_loopback")
    finally:
        check(L.preAlps_hip_set_comm(pl.ALLREDUCE_FN(), pl.EXCHANGE_FN(), None), "set_comm")

    # the library's own loop passes the refusals on and checks ldsol before it starts
    e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, TOL, 100)
    nh = C.c_int(0)
    rc = L.preAlps_ECGSolveMulti(C.byref(e), 2, pB, m, px, m - 1, None, None, None, None, 0, C.byref(nh))
    _refused(L, rc, "preAlps_ECGSolveMulti", "ldsol = %d" % (m - 1))
    rc = L.preAlps_ECGSolveMulti(C.byref(e), 3, pB, m, px, m, None, None, None, None, 0, C.byref(nh))
    _refused(L, rc, entry, "not a multiple of nrhs = 3")

    # a solver that holds two systems
    e, rc = init(4, 2)
    check(rc, entry)
    try:
        one = np.zeros(m)
        _refused(L, L.preAlps_ECGFinalize(C.byref(e), one.ctypes.data_as(pd)), "preAlps_ECGFinalize:", "2 systems",
                 "preAlps_ECGFinalizeMulti")
        rs, li, lr = C.c_int(0), C.c_int(0), C.c_double(0.0)
        rc = L.preAlps_ECGAdvance(C.byref(e), pB, C.byref(rci), 3, C.byref(rs), C.byref(li), C.byref(lr))
        _refused(L, rc, "preAlps_ECGAdvance", "2 systems")
        _refused(L, L.preAlps_ECGFinalizeMulti(C.byref(e), px, m - 1), "preAlps_ECGFinalizeMulti",
                 "ldsol = %d" % (m - 1))
    finally:
        check(L.preAlps_ECGFinalizeMulti(C.byref(e), px, m), "preAlps_ECGFinalizeMulti")
    # nothing of the above has changed what the process can do next
    got = prob.solve_multi(B[:, :2], 4, tol=TOL)
    assert (got.sys_res <= TOL * got.sys_normb).all()
