"""The solution history on the device: the kernels of prealps_amd/csrc/history.hip alone through ctypes against long
double, and preAlps_SolutionHistory* / preAlps_ECGSolveSystemHistory through EcgProblem -- the Galerkin property of the
projection, the bits of the solve it starts, a repeated right-hand side, the ring, a values update, the heat sequence
and the refusals.  Bounds and references: tests/history_ref.py (tests/test_history_ref_cpu.py checks them without a GPU).

Problems as tests/test_gpu_system_solve.py builds them (a few thousand rows at most): P = Poisson 10^3 with part[i] =
(i // 5) % 8; G = the graded S A0 S on 8 contiguous parts, Gupd its second grading; E = elasticity 12 x 10 x 10 with
boxes of 2 x 2 x 2 nodes; U = P built with scale=False; H = the heat matrix I + 5 K on 8 contiguous parts, unscaled.
Right-hand sides: default_rng(20260407).standard_normal((N, 16))."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import history_ref as H

pytestmark = pytest.mark.gpu

TOL = 1e-5
G_RANGE, G_RANGE_2 = (-2.0, 2.0), (1.0, -1.5)
LD = np.longdouble
vp, ci = C.c_void_p, C.c_int

# ---- problems (the operator is process-global in the library: one at a time) ---------------------------------
_open = {}


def _matrix(name):
    from prealps_amd import gen
    if name in ("P", "U"):
        rp, ci_, v = gen.poisson3d_csr(10)
        return rp, ci_, v, ((np.arange(1000) // 5) % 8).astype(np.int32), 8
    if name in ("G", "Gupd"):
        rp, ci_, v = gen.poisson3d_csr(10)
        return rp, ci_, gen.graded_values(rp, ci_, v, *G_RANGE), None, 8
    if name == "H":
        A, _ = H.heat_matrix()
        return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), None, H.HEAT_PARTS
    nn = (12, 10, 10)
    rp, ci_, v = gen.elasticity3d_csr(nn)
    part, P = gen.box_partition_nodes(nn, (2, 2, 2))
    return rp, ci_, v, part, P


def _describe(prob, A0):
    N = prob.N
    return dict(prob=prob, A=A0, absA=abs(A0), n_max=int(np.diff(A0.indptr).max()), N=N,
                B=np.random.default_rng(20260407).standard_normal((N, 16)), lu=spla.splu(A0.tocsc()), cache={})


def _problem(name):
    import prealps_amd as pa
    if name in _open:
        return _open[name]
    for other in list(_open):
        _open.pop(other)["prob"].close()
    rp, ci_, v, part, P = _matrix(name)
    prob = pa.EcgProblem(rp, ci_, v, P, part, scale=name not in ("U", "H"), device=0)
    A0 = sp.csr_matrix((v, ci_, rp), shape=(prob.N, prob.N))
    prob.create_block_jacobi()
    _open[name] = _describe(prob, A0)
    return _open[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for name in list(_open):
        _open.pop(name)["prob"].close()


def _solutions(pb, n=5):
    """The library's own solutions of the first n right-hand sides (computed once, never changed)."""
    if "sol" not in pb["cache"]:
        pb["cache"]["sol"] = np.column_stack([pb["prob"].solve_system(pb["B"][:, j], 4, tol=1e-8).x for j in range(n)])
    return pb["cache"]["sol"]


def _coefficients(X, x0):
    return np.linalg.lstsq(X, x0, rcond=None)[0]      # (enters the bounds by its size only)


def _worst(pb, X, b, x0):
    c = _coefficients(X, x0)
    rho, bound = H.galerkin(pb["A"], pb["absA"], pb["n_max"], X, list(range(X.shape[1])), b, x0, c)
    return float((np.abs(rho) / bound).max()), rho, bound, c


# ---- the kernels alone ------------------------------------------------------------------------------------------
class Dev:
    def __init__(self):
        import prealps_amd
        from prealps_amd.lib import check
        self.L, self.check = prealps_amd.load(), check
        L = self.L
        check(L.preAlps_hip_init(0), "init")
        L.pa_rt_error.restype = C.c_char_p
        L.pa_rt_malloc.restype, L.pa_rt_malloc.argtypes = vp, [C.c_size_t]
        L.pa_rt_free.restype, L.pa_rt_free.argtypes = None, [vp]
        L.pa_rt_h2d.argtypes = [vp, vp, C.c_size_t]
        L.pa_rt_d2h.argtypes = [vp, vp, C.c_size_t]
        L.pa_k_hist_part_doubles.restype = C.c_size_t
        L.pa_k_hist_dots.argtypes = [ci, ci, ci, vp, ci, ci, ci, vp, ci, vp, vp]
        L.pa_k_hist_dots_mapped.argtypes = [ci, ci, ci, vp, ci, ci, ci, vp, vp, vp, ci, vp, vp]
        L.pa_k_hist_combine.argtypes = [ci, ci, ci, vp, ci, ci, ci, vp, vp, ci]
        self.bufs = []
        self.part = self.alloc(L.pa_k_hist_part_doubles() * 8)

    def alloc(self, nbytes):
        d = self.L.pa_rt_malloc(max(nbytes, 8))
        assert d
        self.bufs.append(d)
        return d

    def up(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        self.check(self.L.pa_rt_h2d(d, a.ctypes.data, a.nbytes), "h2d")
        return d

    def down(self, d, n):
        h = np.zeros(n)
        self.check(self.L.preAlps_hip_sync(), "sync")
        self.check(self.L.pa_rt_d2h(h.ctypes.data, d, h.nbytes), "d2h")
        return h

    def free_all_but_part(self):
        self.L.preAlps_hip_sync()
        for d in self.bufs[1:]:
            self.L.pa_rt_free(d)
        self.bufs = self.bufs[:1]

    def close(self):
        self.L.preAlps_hip_sync()
        for d in self.bufs:
            self.L.pa_rt_free(d)
        self.bufs = []


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def _colmajor(V, ld):
    """The (n, k) array V as k columns of ld doubles, NaN in the padding rows."""
    out = np.full((V.shape[1], ld), np.nan)
    out[:, :V.shape[0]] = V.T
    return out


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 4097])
def test_kernels_against_long_double(dev, N):
    rng = np.random.default_rng(N)
    L = dev.L
    case = 0
    for K in (1, 3, 4, 5, 8, 16):
        for q in (1, 2, 4, 5, 16):
            case += 1
            ld = N + (3 if case % 2 else 0)
            cap = min(16, K + case % 3)
            head = (case * 5) % cap                       # a ring that has wrapped whenever head > 0
            X = rng.standard_normal((N, K))
            W = rng.standard_normal((N, q))
            ring = np.full((N, cap), np.nan)              # slots that hold no live column: NaN
            for i in range(K):
                ring[:, (head + i) % cap] = X[:, i]
            d_ring, d_W = dev.up(_colmajor(ring, ld)), dev.up(_colmajor(W, ld))
            d_out = dev.up(np.full(K * q, np.nan))
            # plain dots, twice: the same bits
            got = []
            for _ in range(2):
                assert L.pa_k_hist_dots(N, K, q, d_ring, ld, head, cap, d_W, ld, dev.part, d_out) == 0, L.pa_rt_error()
                got.append(dev.down(d_out, K * q))
            assert got[0].tobytes() == got[1].tobytes(), (K, q)
            g = got[0].reshape(q, K).T
            assert (np.abs(g - H.dots_exact(X, W)) <= H.dots_bound(X, W, N)).all(), (K, q)
            # mapped dots: Xh read through a row map, W a row-major panel divided by dl
            ts = next(t for t in (2, 4, 8, 16) if t >= q)
            src = rng.permutation(N).astype(np.int32)
            dl = rng.uniform(0.5, 2.0, N)
            panel = np.full((N, ts), np.nan)
            panel[:, :q] = W
            d_src, d_dl, d_panel = dev.up(src), dev.up(dl), dev.up(panel)
            got = []
            for _ in range(2):
                assert L.pa_k_hist_dots_mapped(N, K, q, d_ring, ld, head, cap, d_src, d_dl, d_panel, ts, dev.part, d_out) == 0, \
                    L.pa_rt_error()
                got.append(dev.down(d_out, K * q))
            assert got[0].tobytes() == got[1].tobytes(), (K, q)
            Wd = W.astype(LD) / dl.astype(LD)[:, None]
            exact = X[src].astype(LD).T @ Wd
            bound = H.gamma(N + 2) * (np.abs(X[src]).astype(LD).T @ np.abs(Wd))
            assert (np.abs(got[0].reshape(q, K).T - exact) <= bound).all(), (K, q)
            # combine
            c = rng.standard_normal((K, q))
            d_c = dev.up(np.ascontiguousarray(c.T))
            d_x0 = dev.up(np.full((q, ld), np.nan))
            got = []
            for _ in range(2):
                assert L.pa_k_hist_combine(N, K, q, d_ring, ld, head, cap, d_c, d_x0, ld) == 0, L.pa_rt_error()
                got.append(dev.down(d_x0, q * ld))
            assert got[0].tobytes() == got[1].tobytes()
            x0 = got[0].reshape(q, ld)
            assert np.isnan(x0[:, N:]).all()              # the padding rows are not written
            assert (np.abs(x0[:, :N].T - H.combine_exact(X, c)) <= H.combine_bound(X, c)).all(), (K, q)
            dev.free_all_but_part()


def test_the_launchers_refuse_what_does_not_fit(dev):
    L = dev.L
    d = dev.up(np.ones(64 * 16))
    for K, q in ((0, 1), (17, 1), (1, 0), (1, 17)):
        cap = 16
        assert L.pa_k_hist_dots(8, K, q, d, 8, 0, cap, d, 8, dev.part, d) != 0
        assert "pa_k_hist_dots" in L.pa_rt_error().decode()
        assert L.pa_k_hist_dots_mapped(8, K, q, d, 8, 0, cap, d, d, d, 16, dev.part, d) != 0
        assert "pa_k_hist_dots_mapped" in L.pa_rt_error().decode()
        assert L.pa_k_hist_combine(8, K, q, d, 8, 0, cap, d, d, 8) != 0
        assert "pa_k_hist_combine" in L.pa_rt_error().decode()
    assert L.pa_k_hist_dots(8, 4, 2, d, 7, 0, 4, d, 8, dev.part, d) != 0          # ldh below the rows
    assert L.pa_k_hist_dots(8, 4, 2, d, 8, 4, 4, d, 8, dev.part, d) != 0          # head outside the ring
    assert L.pa_k_hist_dots(8, 4, 2, d, 8, 0, 3, d, 8, dev.part, d) != 0          # a ring smaller than K
    assert L.pa_k_hist_dots_mapped(8, 2, 4, d, 8, 0, 2, d, d, d, 2, dev.part, d) != 0   # a panel narrower than q
    dev.L.preAlps_hip_sync()


# ---- the Galerkin property ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P", "G", "E", "U"])
def test_the_projection_is_the_galerkin_projection(name):
    import torch
    pb = _problem(name)
    prob = pb["prob"]
    X = _solutions(pb)
    prob.enable_history(8)
    try:
        prob.history_append(X)
        assert prob.stat("hist_columns") == 5 and prob.stat("hist_capacity") == 8
        assert prob.stat("hist_bytes") == 8.0 * pb["N"] * 8 and prob.stat("hist_appends") == 5
        b = pb["B"][:, 5]
        x0, rank, captured = prob.history_project(b)
        assert rank == 5 and prob.stat("hist_last_rank") == 5
        w, rho, bound, c = _worst(pb, X, b, x0)
        print("%s: worst |rho| / bound = %.3e" % (name, w))
        assert w <= 1.0, (rho, bound)
        assert abs(captured[0] - H.energy_norm(pb["A"], x0) ** 2) <= 1e-9 * captured[0]
        # the best approximation from the span, up to the same bound (the cross term 2 delta^T X^T (b - A x0))
        xs = pb["lu"].solve(b)
        na = np.array([H.energy_norm(pb["A"], X[:, j]) for j in range(5)])
        e0 = H.energy_norm(pb["A"], xs - x0) ** 2
        assert e0 <= H.energy_norm(pb["A"], xs) ** 2 + 2 * float((np.abs(c) * na * bound).sum())
        for i in range(5):
            delta = np.abs(c - np.eye(5)[i])
            assert e0 <= H.energy_norm(pb["A"], xs - X[:, i]) ** 2 + 2 * float((delta * na * bound).sum()), i
        # device tensors and NumPy arrays: the same bits, and two projections agree
        xd, rank_d, cap_d = prob.history_project(torch.from_numpy(b).cuda())
        assert rank_d == 5 and xd.cpu().numpy().tobytes() == x0.tobytes() and cap_d.tobytes() == captured.tobytes()
        assert prob.history_project(b)[0].tobytes() == x0.tobytes()
        # several right-hand sides at once: column j is the projection of column j
        x3, rank3, _ = prob.history_project(pb["B"][:, 5:8])
        assert rank3 == 5 and x3[:, 0].tobytes() == x0.tobytes()
    finally:
        prob.disable_history()
    assert prob.stat("hist_capacity") == 0 and prob.stat("hist_columns") == 0


# ---- bits ---------------------------------------------------------------------------------------------------------
def _same_solve(a, b):
    assert a.iters == b.iters
    assert np.asarray(a.x).tobytes() == np.asarray(b.x).tobytes()
    assert a.res.tobytes() == b.res.tobytes() and a.sys_hist.tobytes() == b.sys_hist.tobytes()
    assert a.sys_res_original.tobytes() == b.sys_res_original.tobytes()


@pytest.mark.parametrize("variant", ["odir", "omin"])
@pytest.mark.parametrize("stop", ["original", "scaled"])
@pytest.mark.parametrize("k", [1, 2])
def test_the_solve_is_the_system_solve_bit_for_bit(k, stop, variant):
    import prealps_amd as pa
    pb = _problem("P")
    prob = pb["prob"]
    alg = pa.ORTHODIR if variant == "odir" else pa.ORTHOMIN
    B1 = pb["B"][:, :k] if k > 1 else pb["B"][:, 0]
    B2 = pb["B"][:, 4:4 + k] if k > 1 else pb["B"][:, 4]
    B2 = B2 + 0.5 * B1                        # (so that the history holds a part of the answer)
    prob.enable_history(8)
    try:
        plain = prob.solve_system(B1, 4, stop=stop, ortho_alg=alg, tol=TOL)
        first = prob.solve_system(B1, 4, stop=stop, ortho_alg=alg, tol=TOL, history=True)
        _same_solve(first, plain)
        assert first.history_rank == 0 and prob.stat("hist_columns") == k
        assert first.sys_res0.tobytes() == first.sys_normb.tobytes()            # a cold start: ||b_j||
        x0, rank, _ = prob.history_project(B2)
        assert rank == k
        ref = prob.solve_system(B2, 4, x0=x0, stop=stop, ortho_alg=alg, tol=TOL)
        got = prob.solve_system(B2, 4, stop=stop, ortho_alg=alg, tol=TOL, history=True)
        _same_solve(got, ref)
        assert got.history_rank == k and prob.stat("hist_columns") == 2 * k
        assert (got.sys_res0 < got.sys_normb).all()
    finally:
        prob.disable_history()


# ---- a repeated right-hand side --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["H", "P"])
def test_a_repeated_right_hand_side(name):
    pb = _problem(name)
    prob = pb["prob"]
    b = pb["B"][:, 0]
    prob.enable_history(8)
    try:
        first = prob.solve_system(b, 4, tol=TOL, history=True)
        again = prob.solve_system(b, 4, tol=TOL, history=True)
        print("%s: start residual / (tol ||b||) = %.3f, %d iterations" % (name, again.sys_res0[0] / (TOL * np.linalg.norm(b)),
                                                                         again.iters))
        assert again.history_rank == 1
        assert again.sys_res0[0] <= 8 * TOL * np.linalg.norm(b)
        assert again.iters <= 2 and first.iters > 2
        # (a start that already meets the threshold comes back as x, and nothing is appended)
        assert prob.stat("hist_columns") == (1 if again.iters == 0 else 2)
    finally:
        prob.disable_history()


# ---- the ring -----------------------------------------------------------------------------------------------------
def test_a_full_ring_holds_the_last_columns():
    pb = _problem("P")
    prob = pb["prob"]
    X = _solutions(pb)
    b = pb["B"][:, 5]
    prob.enable_history(3)
    try:
        for j in range(5):
            prob.history_append(X[:, j])
        assert prob.stat("hist_columns") == 3 and prob.stat("hist_appends") == 5
        xa, ra, _ = prob.history_project(b)
        prob.enable_history(3)                      # replaces the ring: a fresh one that holds the last three
        prob.history_append(X[:, 2:])
        assert prob.stat("hist_columns") == 3
        xb, rb, _ = prob.history_project(b)
        assert ra == 3 and rb == 3
        wa, _, bound_a, _ = _worst(pb, X[:, 2:], b, xa)
        wb, _, bound_b, _ = _worst(pb, X[:, 2:], b, xb)
        assert wa <= 1.0 and wb <= 1.0
        # both lie within ||bound|| / sqrt(lambda_min(Gs)) of the exact projection, in the energy norm
        Xs = X[:, 2:] / np.array([H.energy_norm(pb["A"], X[:, j]) for j in range(2, 5)])
        lam = np.linalg.eigvalsh(Xs.T @ (pb["A"] @ Xs))[0]
        room = (float(np.linalg.norm(bound_a.astype(float))) + float(np.linalg.norm(bound_b.astype(float)))) / np.sqrt(lam)
        assert H.energy_norm(pb["A"], xa - xb) <= room
        # more columns than the capacity at once: the last three again
        prob.clear_history()
        assert prob.stat("hist_columns") == 0
        prob.history_append(X)
        assert prob.stat("hist_columns") == 3
        xc, rc, _ = prob.history_project(b)
        assert rc == 3 and _worst(pb, X[:, 2:], b, xc)[0] <= 1.0
    finally:
        prob.disable_history()


# ---- a values update ------------------------------------------------------------------------------------------------
def test_the_gram_matrix_follows_a_values_update():
    from prealps_amd import gen
    pb = _problem("Gupd")
    prob = pb["prob"]
    X = _solutions(pb)
    rp, ci_, v0 = gen.poisson3d_csr(10)
    v2 = gen.graded_values(rp, ci_, v0, *G_RANGE_2)
    A2 = sp.csr_matrix((v2, ci_, rp), shape=(pb["N"], pb["N"]))
    new = dict(A=A2, absA=abs(A2), n_max=pb["n_max"])
    b = pb["B"][:, 5]
    prob.enable_history(8)
    try:
        prob.history_append(X)
        assert prob.stat("hist_gram_refreshes") == 0 and prob.stat("hist_values_epoch") == prob.stat("op_values_epoch")
        prob.update_values(v2, precond="refactor")
        assert prob.stat("hist_values_epoch") < prob.stat("op_values_epoch")        # lazy: nothing has happened yet
        x0, rank, _ = prob.history_project(b)
        assert rank == 5 and prob.stat("hist_gram_refreshes") == 1
        assert prob.stat("hist_values_epoch") == prob.stat("op_values_epoch")
        w_new = _worst(new, X, b, x0)[0]
        w_old = _worst(pb, X, b, x0)[0]
        print("values update: worst |rho| / bound against the new matrix %.3e, against the old one %.3e" % (w_new, w_old))
        assert w_new <= 1.0 and w_old > 100.0
        prob.history_project(b)
        prob.history_append(X[:, 0])
        assert prob.stat("hist_gram_refreshes") == 1
    finally:
        prob.disable_history()
        _open.pop("Gupd")["prob"].close()            # (its cache describes the old values)


# ---- the heat sequence ----------------------------------------------------------------------------------------------
def test_the_heat_sequence():
    ref = H.heat_reference()
    pb = _problem("H")
    prob = pb["prob"]
    prob.enable_history(8)
    try:
        u = np.zeros(pb["N"])
        iters, cold = [], []
        for n in range(1, H.HEAT_STEPS + 1):
            b = H.heat_rhs(u, n)
            if 8 <= n <= 15:
                cold.append(prob.solve_system(b, H.HEAT_T, stop="scaled", tol=H.HEAT_TOL).iters)
            r = prob.solve_system(b, H.HEAT_T, stop="scaled", tol=H.HEAT_TOL, history=True)
            iters.append(r.iters)
            u = r.x
        print("heat: iterations per step with history %s (restatement %s), cold over steps 8..15 %s" % (iters, ref["hist"], cold))
        for n, (a, e) in enumerate(zip(iters, ref["hist"]), 1):
            assert abs(a - e) <= 1, (n, a, e)
        assert sum(iters[7:15]) <= 0.5 * sum(cold), (iters, cold)
        assert prob.stat("hist_columns") == 8 and prob.stat("hist_projections") == H.HEAT_STEPS
    finally:
        prob.disable_history()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_and_leave_the_history_alone():
    import prealps_amd as pa
    pb = _problem("P")
    prob = pb["prob"]
    L = prob.L
    N = pb["N"]
    X = _solutions(pb)
    b = np.ascontiguousarray(pb["B"][:, 5])
    prob.enable_history(4)
    try:
        prob.history_append(X[:, :3])
        before = prob.history_project(b)[0].tobytes()
        out, rank = np.zeros(N), C.c_int()
        wide = np.asfortranarray(np.ones((N, 17)))
        bad = X[:, 0].copy()
        bad[N // 2] = np.nan
        binf = b.copy()
        binf[3] = np.inf
        e = prob.new_ecg(4, tol=TOL)
        calls = [
            ("preAlps_SolutionHistoryCreate", lambda: L.preAlps_SolutionHistoryCreate(0), "capacity"),
            ("preAlps_SolutionHistoryCreate", lambda: L.preAlps_SolutionHistoryCreate(17), "capacity"),
            ("preAlps_SolutionHistoryAppend", lambda: L.preAlps_SolutionHistoryAppend(0, b.ctypes.data, N, 0), "nrhs"),
            ("preAlps_SolutionHistoryAppend", lambda: L.preAlps_SolutionHistoryAppend(17, wide.ctypes.data, N, 0), "nrhs"),
            ("preAlps_SolutionHistoryAppend", lambda: L.preAlps_SolutionHistoryAppend(1, b.ctypes.data, N - 1, 0), "ldx"),
            ("preAlps_SolutionHistoryAppend", lambda: L.preAlps_SolutionHistoryAppend(1, None, N, 0), "NULL"),
            ("preAlps_SolutionHistoryAppend", lambda: L.preAlps_SolutionHistoryAppend(1, b.ctypes.data, N, 4), "flags"),
            ("preAlps_SolutionHistoryAppend", lambda: L.preAlps_SolutionHistoryAppend(1, bad.ctypes.data, N, 0), "not finite"),
            ("preAlps_SolutionHistoryProject", lambda: L.preAlps_SolutionHistoryProject(1, binf.ctypes.data, N, out.ctypes.data, N,
                                                                                      0, 0.0, C.byref(rank), None), "not finite"),
            ("preAlps_SolutionHistoryProject", lambda: L.preAlps_SolutionHistoryProject(1, b.ctypes.data, N, out.ctypes.data,
                                                                                      N - 1, 0, 0.0, C.byref(rank), None), "ldx0"),
            ("preAlps_SolutionHistoryProject", lambda: L.preAlps_SolutionHistoryProject(1, b.ctypes.data, N, None, N, 0, 0.0,
                                                                                      C.byref(rank), None), "NULL"),
            ("preAlps_ECGSolveSystemHistory", lambda: L.preAlps_ECGSolveSystemHistory(
                C.byref(e), 3, wide.ctypes.data, N, wide.ctypes.data, N, 0, 0.0, None, None, None, None, None, None, None, 0,
                None), "multiple"),
            ("preAlps_ECGSolveSystemHistory", lambda: L.preAlps_ECGSolveSystemHistory(
                C.byref(e), 1, binf.ctypes.data, N, out.ctypes.data, N, 0, 0.0, None, None, None, None, None, None, None, 0,
                None), "not finite"),
        ]
        for entry, call, reason in calls:
            assert call() != 0, (entry, reason)
            msg = (L.preAlps_hip_last_error() or b"").decode()
            assert msg.startswith(entry + ":") and reason in msg, (entry, reason, msg)
            assert prob.stat("hist_columns") == 3 and prob.stat("hist_capacity") == 4, (entry, reason)
        assert prob.history_project(b)[0].tobytes() == before
        prob.disable_history()
        with pytest.raises(pa.PreAlpsError, match="preAlps_SolutionHistoryAppend.*no solution history"):
            prob.history_append(b)
        with pytest.raises(pa.PreAlpsError, match="preAlps_ECGSolveSystemHistory.*no solution history"):
            prob.solve_system(b, 4, history=True)
    finally:
        prob.disable_history()
