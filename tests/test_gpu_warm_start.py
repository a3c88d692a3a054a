"""The ECG iteration started from an initial guess (preAlps_ECGInitializeGuess / preAlps_ECGSolveGuess,
EcgProblem.solve(..., x0=) and solve_multi(..., X0=)), for one and several systems.

Problems: those of test_gpu_multi_rhs.py -- P = Poisson 10^3, 8 contiguous parts; E = elasticity on 12 x 10 x 10 nodes
with boxes of 2 x 2 x 2 nodes -- and its right-hand sides B = default_rng(20260407).standard_normal((m, 16)).  The
checker is this file's own copy of that file's NumPy restatement of Orthodir on the library's scaled and permuted
matrix (local_csr), extended by the start: X0 split by the placement rule, R0 = the split of B - (group sums of A X0)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

TOL = 1e-5
RTOL_HIST = 1e-8          # Poisson histories against another fp64 implementation
PD = C.POINTER(C.c_double)


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
    absA = sp.csr_matrix((np.abs(lv), lci, lrp), shape=(prob.m, prob.M))
    rowpos = np.asarray(prob.rowpos, dtype=np.int64)
    rng = np.random.default_rng(20260407)
    _open[name] = dict(prob=prob, A=A, absA=absA, n_max=int(np.diff(lrp).max()), rowpos=rowpos,
                       B=rng.standard_normal((prob.m, 16)), cache={})
    return _open[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for name in list(_open):
        _open.pop(name)["prob"].close()


def _variants():
    import prealps_amd as pa
    return {"odir": (pa.ORTHODIR, pa.NO_BS_RED), "omin": (pa.ORTHOMIN, pa.NO_BS_RED),
            "odir-adapt": (pa.ORTHODIR, pa.ADAPT_BS), "omin-adapt": (pa.ORTHOMIN, pa.ADAPT_BS)}


def _cached(pb, key, make):
    """Results that several tests share (cold solves, the guesses): computed once, never changed."""
    if key not in pb["cache"]:
        pb["cache"][key] = make()
    return pb["cache"][key]


def _cold(pb, k, s, variant="odir"):
    alg, red = _variants()[variant]
    return _cached(pb, ("cold", k, s, variant),
                   lambda: pb["prob"].solve_multi(pb["B"][:, :k], k * s, ortho_alg=alg, bs_red=red, tol=TOL))


def _coarse_guess(pb, k, s):
    """The library's own tol = 1e-3 solution of the k systems."""
    return _cached(pb, ("guess", k, s), lambda: pb["prob"].solve_multi(pb["B"][:, :k], k * s, tol=1e-3).x.copy())


# ---- the NumPy restatement of Orthodir, with the start -------------------------------------------------------
def _block_inverses(pb):
    return _cached(pb, "inv", lambda: [np.linalg.inv(pb["A"][r0:r1, r0:r1].toarray())
                                       for r0, r1 in zip(pb["rowpos"][:-1], pb["rowpos"][1:])])


def _split(V, rowpos, s):
    """(N x k) -> (N x k*s): a row of part p puts V(row, j) into column j*s + p % s, zero elsewhere."""
    N, k = V.shape
    out = np.zeros((N, k * s))
    for p in range(len(rowpos) - 1):
        for j in range(k):
            out[rowpos[p]:rowpos[p + 1], j * s + p % s] = V[rowpos[p]:rowpos[p + 1], j]
    return out


def _restate(pb, B, s, X0=None, tol=TOL, max_iter=500):
    """Orthodir on R0 = the split of the k columns of B into s columns each or, from a guess, on X = split(X0) and
    R0 = split(B - group sums of A X).  Returns the per-system history (iterations x k, absolute), the k solutions,
    ||b_j|| and the start residual norms g0_j."""
    A, rowpos, inv = pb["A"], pb["rowpos"], _block_inverses(pb)
    N, k = B.shape
    t, nparts = k * s, len(rowpos) - 1

    def precond(X):
        Y = np.empty_like(X)
        for p in range(nparts):
            Y[rowpos[p]:rowpos[p + 1]] = inv[p] @ X[rowpos[p]:rowpos[p + 1]]
        return Y

    if X0 is None:
        X, R = np.zeros((N, t)), _split(B, rowpos, s)
    else:
        X = _split(X0, rowpos, s)
        R = _split(B - (A @ X).reshape(N, k, s).sum(axis=2), rowpos, s)
    nb = np.linalg.norm(B, axis=0)
    g0 = np.sqrt((R ** 2).reshape(N, k, s).sum(axis=(0, 2)))
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
    return np.array(hist), X.reshape(N, k, s).sum(axis=2), nb, g0


def _assert_count_is_safe(hist, nb):
    """The restatement's own history decides the count with room to spare, so a rounding difference between it and
    the library cannot move it: under 0.99 of the threshold at the last iteration, over 1.01 at the one before."""
    last = (hist[-1] / (TOL * nb)).max()
    assert last < 0.99, last
    if len(hist) > 1:
        before = (hist[-2] / (TOL * nb)).max()
        assert before > 1.01, before


# ---- what the start must satisfy -----------------------------------------------------------------------------
def _start_reference(pb, B, X0):
    """NumPy's r0 = B - A X0 and the a-priori elementwise bound on the library's deviation from it:
    4 (n_max + 2) 2^-53 (|A| |X0| + |B|), n_max the longest row.  A row of A X0 is a sum of at most n_max products,
    in any order and with or without fused multiply-adds, here and in NumPy: each is within (n_max + 1) u (|A| |X0|)
    of the exact value to first order; the group sum adds zeros, the subtraction one more rounding of at most
    u (|A| |X0| + |B|).  Twice that for the two sides, and a factor 2 for the higher-order terms: 4 (n_max + 2) u."""
    r0 = B - pb["A"] @ X0
    bound = 4.0 * (pb["n_max"] + 2) * 2.0 ** -53 * (pb["absA"] @ np.abs(X0) + np.abs(B))
    return r0, bound


def _check_start_residuals(pb, B, X0, g0):
    r0, bound = _start_reference(pb, B, X0)
    want = np.linalg.norm(r0, axis=0)
    slack = np.linalg.norm(bound, axis=0) + 1e-14 * want
    print("g0", g0, "reference", want, "slack", slack)
    assert (np.abs(g0 - want) <= slack).all(), (g0, want, slack)


# ---- 1. no guess and a zero guess are today's solve ------------------------------------------------------------
@pytest.mark.parametrize("variant", ["odir", "omin"])
@pytest.mark.parametrize("t", [1, 2, 4, 8])
def test_a_zero_guess_is_the_single_system_solve(t, variant):
    """b - A 0 = b exactly and 0 + x = x: the same bytes in res, bs and x.  A scratch panel left dirty by the start
    or a start that reorders the iteration would show here."""
    pb = _problem("E")
    prob = pb["prob"]
    alg, red = _variants()[variant]
    b = np.ascontiguousarray(pb["B"][:, 0])
    one = prob.solve(b, t, ortho_alg=alg, bs_red=red, tol=TOL)
    got = prob.solve(b, t, ortho_alg=alg, bs_red=red, tol=TOL, x0=np.zeros(prob.m))
    assert got.iters == one.iters > 0 and got.x.shape == (prob.m,)
    assert got.res.tobytes() == one.res.tobytes() and got.bs.tobytes() == one.bs.tobytes()
    assert got.x.tobytes() == one.x.tobytes()
    assert got.normb == one.normb and got.sys_res0[0] == pytest.approx(one.normb, rel=1e-14)
    # no guess at all: the path of today
    none = prob.solve(b, t, ortho_alg=alg, bs_red=red, tol=TOL, x0=None)
    assert none.res.tobytes() == one.res.tobytes() and none.x.tobytes() == one.x.tobytes() and none.sys_res0 is None


@pytest.mark.parametrize("variant", ["odir", "omin"])
@pytest.mark.parametrize("k,s", [(2, 2), (4, 1), (3, 1)])
def test_a_zero_guess_is_the_multi_system_solve(k, s, variant):
    """The same for several systems; the sums of b_j^2 must also come out of the start kernel in the order of
    k_multi_start."""
    pb = _problem("E")
    prob = pb["prob"]
    alg, red = _variants()[variant]
    B = pb["B"][:, :k]
    one = prob.solve_multi(B, k * s, ortho_alg=alg, bs_red=red, tol=TOL)
    got = prob.solve_multi(B, k * s, ortho_alg=alg, bs_red=red, tol=TOL, X0=np.zeros((prob.m, k)))
    assert got.iters == one.iters > 0
    assert got.res.tobytes() == one.res.tobytes() and got.bs.tobytes() == one.bs.tobytes()
    assert got.x.tobytes() == one.x.tobytes()
    assert got.sys_hist.tobytes() == one.sys_hist.tobytes()
    assert got.sys_normb.tobytes() == one.sys_normb.tobytes() and got.normb == one.normb
    np.testing.assert_allclose(got.sys_res0, one.sys_normb, rtol=1e-14)     # (R0 = split(B): other sums, same norm)
    assert one.sys_res0 is None


# ---- 2. the start itself ---------------------------------------------------------------------------------------
def _panel(L, d, m):
    """Host copy of a solver panel (d: the descriptor pointer of the solver object)."""
    n = d.contents.info.n
    out = np.zeros((m, n), order="F")
    assert L.preAlps_hip_panel_to_host(d, n, out.ctypes.data_as(PD), max(m, 1)) == 0
    return out


@pytest.mark.parametrize("k,s", [(1, 4), (2, 2), (3, 1), (3, 4), (16, 1)])
@pytest.mark.parametrize("name", ["P", "E"])
def test_the_start_splits_the_guess_and_its_residual(name, k, s):
    """Strides 4, 4, 4 (t = 3, padded), 16 (t = 12, padded), 16."""
    import prealps_amd as pa
    from prealps_amd.lib import check
    pb = _problem(name)
    prob, L, m, rowpos = pb["prob"], pb["prob"].L, pb["prob"].m, pb["rowpos"]
    t = k * s
    B = np.asfortranarray(pb["B"][:, :k])
    X0 = np.asfortranarray(np.random.default_rng(99 + 16 * k + s).standard_normal((m, k)))
    check(L.preAlps_hip_prepare_operator(t), "prepare")
    e = prob.new_ecg(t, pa.ORTHODIR, pa.NO_BS_RED, TOL, 100)
    rci = C.c_int(0)
    check(L.preAlps_ECGInitializeGuess(C.byref(e), k, B.ctypes.data_as(PD), m, X0.ctypes.data_as(PD), m,
                                       C.byref(rci)), "preAlps_ECGInitializeGuess")
    sol = np.zeros((m, k), order="F")
    try:
        X, R = _panel(L, e.X, m), _panel(L, e.R, m)
        g0, nb = np.zeros(k), np.zeros(k)
        check(L.preAlps_ECGSystemResiduals(C.byref(e), g0.ctypes.data_as(PD), nb.ctypes.data_as(PD)), "residuals")
        res, normb, it = e.res, e.normb, e.iter
    finally:
        check(L.preAlps_ECGFinalizeMulti(C.byref(e), sol.ctypes.data_as(PD), m), "preAlps_ECGFinalizeMulti")
    assert X.shape == (m, t) and R.shape == (m, t) and it == 0
    live = _split(np.ones((m, k)), rowpos, s) != 0.0
    # X: x0_j in the live column of every row, zero elsewhere, so the sum of a system's columns is x0_j bit for bit
    assert (X[~live] == 0.0).all()
    assert X.reshape(m, k, s).sum(axis=2).tobytes() == np.ascontiguousarray(X0).tobytes()
    assert X.tobytes(order="C") == _split(X0, rowpos, s).tobytes(order="C")
    # R: the same pattern, within the a-priori bound of NumPy's B - A X0
    assert (R[~live] == 0.0).all()
    r0, bound = _start_reference(pb, B, X0)
    dev = np.abs(R.reshape(m, k, s).sum(axis=2) - r0)
    print(name, k, s, "largest deviation / bound", (dev / bound).max())
    assert (dev <= bound).all(), (dev / bound).max()
    # norms
    np.testing.assert_allclose(nb, np.linalg.norm(B, axis=0), rtol=1e-14)
    assert normb == pytest.approx(np.linalg.norm(B), rel=1e-14)
    _check_start_residuals(pb, B, X0, g0)
    assert res ** 2 == pytest.approx((g0 ** 2).sum(), rel=1e-13)
    # finalised without an iteration: the guess comes back bit for bit
    assert sol.tobytes(order="F") == X0.tobytes(order="F")


# ---- 3. warm histories follow the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("k,s", [(1, 1), (1, 4), (2, 2), (4, 1), (3, 1), (8, 1), (16, 1), (3, 4)])
def test_warm_histories_follow_the_restatement(k, s):
    """P, Orthodir, from the library's own tol = 1e-3 solution on to 1e-5."""
    pb = _problem("P")
    B = pb["B"][:, :k]
    X0 = _coarse_guess(pb, k, s)
    got = pb["prob"].solve_multi(B, k * s, tol=TOL, X0=X0)
    hist, x, nb, g0 = _restate(pb, B, s, X0=X0)
    cold = _cold(pb, k, s)
    print(k, s, "warm", got.iters, "restatement", len(hist), "cold", cold.iters)
    _assert_count_is_safe(hist, nb)
    assert got.iters == len(hist) == len(got.res)
    assert got.sys_hist.shape == (got.iters, k) and got.x.shape == (pb["prob"].m, k)
    np.testing.assert_allclose(got.sys_normb, nb, rtol=1e-14)
    np.testing.assert_allclose(got.sys_hist, hist, rtol=RTOL_HIST)
    _check_start_residuals(pb, B, X0, got.sys_res0)
    assert got.iters < cold.iters


# ---- 4. every variant, warm --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["odir", "omin", "odir-adapt", "omin-adapt"])
@pytest.mark.parametrize("k,s", [(4, 1), (2, 2), (1, 4)])
@pytest.mark.parametrize("name", ["P", "E"])
def test_every_variant_goes_on_from_the_guess(name, k, s, variant):
    """At the stop every system is under its own threshold, the true residual obeys the sqrt(s) bound (factor 4.0
    and 1e-12 as in test_gpu_multi_rhs.py), and the warm solve takes fewer iterations than the cold one."""
    pb = _problem(name)
    alg, red = _variants()[variant]
    B = pb["B"][:, :k]
    X0 = _coarse_guess(pb, k, s)
    got = pb["prob"].solve_multi(B, k * s, ortho_alg=alg, bs_red=red, tol=TOL, max_iter=1000, X0=X0)
    cold = _cold(pb, k, s, variant)
    true = np.linalg.norm(B - pb["A"] @ got.x, axis=0)
    print(name, k, s, variant, "warm", got.iters, "cold", cold.iters, "sys_res/normb", got.sys_res / got.sys_normb,
          "true/sys_res", true / got.sys_res)
    assert (got.sys_res <= TOL * got.sys_normb).all(), (got.sys_res, got.sys_normb)
    assert (true <= 4.0 * np.sqrt(s) * got.sys_res + 1e-12).all(), (true, got.sys_res)
    assert 0 < got.iters < cold.iters and len(got.res) == got.iters == len(got.sys_hist)


# ---- 5. a system that starts converged beside systems that start from zero --------------------------------------
@pytest.mark.parametrize("variant", ["odir", "omin"])
@pytest.mark.parametrize("k,s", [(2, 2), (4, 2), (3, 1), (8, 1)])
def test_a_converged_system_beside_cold_ones(k, s, variant):
    """P.  System 0 starts from the library's tol = 1e-7 solution, the others from zero: a small start residual is
    no error, system 0 stays converged at every stopping test, and the count is the restatement's."""
    pb = _problem("P")
    prob = pb["prob"]
    alg, red = _variants()[variant]
    B = pb["B"][:, :k]
    x00 = _cached(pb, "fine0", lambda: prob.solve_multi(pb["B"][:, :1], 4, tol=1e-7).x[:, 0].copy())
    X0 = np.zeros((prob.m, k))
    X0[:, 0] = x00
    got = prob.solve_multi(B, k * s, ortho_alg=alg, bs_red=red, tol=TOL, X0=X0)
    hist, x, nb, g0 = _restate(pb, B, s, X0=X0)
    true = np.linalg.norm(B - pb["A"] @ got.x, axis=0)
    print(k, s, variant, "iters", got.iters, "restatement", len(hist), "system 0 at most",
          (got.sys_hist[:, 0] / got.sys_normb[0]).max(), "restatement", (hist[:, 0] / nb[0]).max())
    _assert_count_is_safe(hist, nb)
    assert got.sys_res0[0] <= 1e-7 * got.sys_normb[0] * 4.0 and (got.sys_res0[1:] == got.sys_normb[1:]).all()
    assert (got.sys_res <= TOL * got.sys_normb).all(), (got.sys_res, got.sys_normb)
    assert (true <= 4.0 * np.sqrt(s) * got.sys_res + 1e-12).all(), (true, got.sys_res)
    assert (got.sys_hist[:, 0] <= TOL * got.sys_normb[0]).all(), got.sys_hist[:, 0] / got.sys_normb[0]
    assert got.iters == len(hist)


# ---- 6. already converged ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", [(2, 2), (1, 4)])
def test_a_converged_guess_comes_back_without_an_iteration(k, s):
    pb = _problem("P")
    prob = pb["prob"]
    B = pb["B"][:, :k]
    X0 = prob.solve_multi(B, k * s, tol=1e-8).x.copy()
    got = prob.solve_multi(B, k * s, tol=TOL, X0=X0)
    assert got.iters == 0 and len(got.res) == 0 and len(got.bs) == 0 and got.sys_hist.shape == (0, k)
    assert got.x.tobytes(order="F") == np.asfortranarray(X0).tobytes(order="F")
    assert (got.sys_res0 <= TOL * got.sys_normb).all() and (got.sys_res0 > 0.0).all()
    _check_start_residuals(pb, B, X0, got.sys_res0)
    np.testing.assert_array_equal(got.sys_res, got.sys_res0)
    if k == 1:
        one = prob.solve(B[:, 0], s, tol=TOL, x0=X0[:, 0])
        assert one.iters == 0 and one.x.tobytes() == np.ascontiguousarray(X0[:, 0]).tobytes()


# ---- 7. the caller's own loop ------------------------------------------------------------------------------------
def test_the_callers_loop_goes_on_from_the_guess():
    """(k, s) = (2, 2) on P through InitializeGuess, the RCI calls in the order of the reference driver,
    preAlps_ECGSystemResiduals after each stopping test and FinalizeMulti."""
    import prealps_amd as pa
    from prealps_amd.lib import check
    pb = _problem("P")
    prob, L = pb["prob"], pb["prob"].L
    k, s, m = 2, 2, pb["prob"].m
    B = np.asfortranarray(pb["B"][:, :k])
    X0 = np.asfortranarray(_coarse_guess(pb, k, s))
    want = prob.solve_multi(B, k * s, tol=TOL, X0=X0)
    e = prob.new_ecg(k * s, pa.ORTHODIR, pa.NO_BS_RED, TOL, 1000)
    rci, stop = C.c_int(0), C.c_int(0)
    check(L.preAlps_ECGInitializeGuess(C.byref(e), k, B.ctypes.data_as(PD), m, X0.ctypes.data_as(PD), m,
                                       C.byref(rci)), "init")
    nb, g0 = np.zeros(k), np.zeros(k)
    check(L.preAlps_ECGSystemResiduals(C.byref(e), g0.ctypes.data_as(PD), nb.ctypes.data_as(PD)), "normb")
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
            check(L.preAlps_ECGSystemResiduals(C.byref(e), g.ctypes.data_as(PD), None), "residuals")
            hist.append(g)
            if stop.value == 1:
                break
            check(L.preAlps_BlockJacobiApply(e.AP, e.Z), "apply")
    iters = e.iter
    x = np.zeros((m, k), order="F")
    check(L.preAlps_ECGFinalizeMulti(C.byref(e), x.ctypes.data_as(PD), m), "finalize")
    assert iters == want.iters == len(hist) and 0 < iters < _cold(pb, k, s).iters
    np.testing.assert_array_equal(nb, want.sys_normb)
    np.testing.assert_array_equal(g0, want.sys_res0)
    np.testing.assert_allclose(np.array(hist), want.sys_hist, rtol=1e-8)
    np.testing.assert_allclose(x, want.x, rtol=1e-8, atol=1e-8 * np.abs(want.x).max())


# ---- 8. refusals -------------------------------------------------------------------------------------------------
def _refused(L, rc, entry, *reasons):
    assert rc != 0
    msg = L.preAlps_hip_last_error().decode()
    assert entry in msg, msg
    for r in reasons:
        assert r in msg, msg


def test_refusals_name_the_entry_point_and_the_reason():
    import prealps_amd as pa
    from prealps_amd.lib import check
    pb = _problem("P")
    prob, L, m = pb["prob"], pb["prob"].L, pb["prob"].m
    B = np.asfortranarray(pb["B"][:, :2])
    X0 = np.asfortranarray(_coarse_guess(pb, 2, 2))
    rci = C.c_int(0)

    def init(rhs=B, x0=X0, ldx0=m, alg=pa.ORTHODIR, t=4, k=2):
        e = prob.new_ecg(t, alg, pa.NO_BS_RED, TOL, 100)
        return e, L.preAlps_ECGInitializeGuess(C.byref(e), k, rhs.ctypes.data_as(PD), m, x0.ctypes.data_as(PD), ldx0,
                                               C.byref(rci))

    entry = "preAlps_ECGInitializeGuess"
    _refused(L, init(ldx0=m - 1)[1], entry, "ldx0 = %d" % (m - 1))
    bad = X0.copy(order="F")
    bad[m // 2, 1] = np.nan
    _refused(L, init(x0=bad)[1], entry, "system 1", "not finite")
    # exactly zero beside a live one: b_1 = A e_i and x0_1 = e_i, a product of one entry per row, which is exact
    i = m // 3
    unit = np.zeros(m)
    unit[i] = 1.0
    Bz, Xz = B.copy(order="F"), X0.copy(order="F")
    Bz[:, 1] = pb["A"] @ unit
    Xz[:, 1] = unit
    _refused(L, init(rhs=Bz, x0=Xz)[1], entry, "system 1 starts with a zero residual")
    # what preAlps_ECGInitializeMulti refuses, under this entry's name
    _refused(L, init(k=3)[1], entry, "not a multiple of nrhs = 3")
    _refused(L, init(k=0)[1], entry, "nrhs = 0")
    _refused(L, init(t=16, k=1)[1], entry, "size: 8", "enlarging factor per system: 16")
    Z = B.copy(order="F")
    Z[:, 1] = 0.0
    _refused(L, init(rhs=Z)[1], entry, "right-hand side 1 has norm zero")
    _refused(L, init(alg=pa.ORTHODIR_FUSED)[1], entry, "ORTHODIR_FUSED")
    try:
        check(L.preAlps_hip_set_world(0, 2), "set_world")
        _refused(L, init()[1], entry, "single process", "2 processes")
    finally:
        check(L.preAlps_hip_set_world(0, 1), "set_world")

    # the library's own loop passes the refusals on and checks ldsol before it starts
    x = np.zeros((m, 2), order="F")
    px = x.ctypes.data_as(PD)
    e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, TOL, 100)
    nh = C.c_int(0)
    rc = L.preAlps_ECGSolveGuess(C.byref(e), 2, B.ctypes.data_as(PD), m, X0.ctypes.data_as(PD), m, px, m - 1,
                                 None, None, None, None, None, 0, C.byref(nh))
    _refused(L, rc, "preAlps_ECGSolveGuess", "ldsol = %d" % (m - 1))
    rc = L.preAlps_ECGSolveGuess(C.byref(e), 2, B.ctypes.data_as(PD), m, X0.ctypes.data_as(PD), m - 1, px, m,
                                 None, None, None, None, None, 0, C.byref(nh))
    _refused(L, rc, entry, "ldx0 = %d" % (m - 1))

    # preAlps_ECGAdvance restarts from the right-hand side alone: refused on a solver started from a guess,
    # for one system as for several
    for k, t in ((2, 4), (1, 4)):
        e, rc = init(rhs=np.asfortranarray(B[:, :k]), x0=np.asfortranarray(X0[:, :k]), t=t, k=k)
        check(rc, entry)
        try:
            rs, li, lr = C.c_int(0), C.c_int(0), C.c_double(0.0)
            rc = L.preAlps_ECGAdvance(C.byref(e), B.ctypes.data_as(PD), C.byref(rci), 3, C.byref(rs), C.byref(li),
                                      C.byref(lr))
            _refused(L, rc, "preAlps_ECGAdvance", "initial guess", "x0")
        finally:
            check(L.preAlps_ECGFinalizeMulti(C.byref(e), px, m), "preAlps_ECGFinalizeMulti")
    # nothing of the above has changed what the process can do next
    got = prob.solve_multi(B, 4, tol=TOL)
    assert (got.sys_res <= TOL * got.sys_normb).all()
    assert got.res.tobytes() == _cold(pb, 2, 2).res.tobytes()
