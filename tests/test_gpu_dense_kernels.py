"""Kernel-level parity of the tall-skinny panel kernels (Gram products, Z update, the fused
triangular solve + iterate update) against numpy on the host, through the C ABI
(preAlps_hip_panel_gram / _update / _trsm_update launch what the solver launches).  Covers the
register-tiled kernels (panel stride 2, 4) and the matrix-core ones (stride 8, 16), column
counts off the stride (3, 5, 12), and row counts that are not multiples of any tile."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Panels:
    def __init__(self):
        import prealps_amd
        from prealps_amd.lib import check
        self.L, self.check = prealps_amd.load(), check
        check(self.L.preAlps_hip_init(0), "init")
        self.live = []

    def up(self, H, t):
        from prealps_amd.lib import CPLM_Mat_Dense_t
        m, n = H.shape
        d = CPLM_Mat_Dense_t()
        self.check(self.L.preAlps_hip_panel_alloc(C.byref(d), m, n, m, n, t), "alloc")
        Hf = np.asfortranarray(H)
        self.check(self.L.preAlps_hip_panel_from_host(C.byref(d), t, _pd(Hf), m), "h2d")
        self.live.append(d)
        return d

    def down(self, d, t):
        out = np.zeros((d.info.m, d.info.n), order="F")
        self.check(self.L.preAlps_hip_panel_to_host(C.byref(d), t, _pd(out), max(d.info.m, 1)), "d2h")
        return out

    def close(self):
        for d in self.live:
            self.L.preAlps_hip_panel_free(C.byref(d))


@pytest.fixture
def panels():
    p = Panels()
    yield p
    p.close()


@pytest.mark.parametrize("m", [1, 1000, 40961])
@pytest.mark.parametrize("t,na1", [(2, 2), (4, 0), (4, 4), (3, 2), (8, 0), (8, 8), (5, 3), (16, 0), (16, 16), (12, 7)])
def test_gram(panels, m, t, na1):
    rng = np.random.default_rng(m + 31 * t + na1)
    A0, B = rng.standard_normal((m, t)), rng.standard_normal((m, t))
    A1 = rng.standard_normal((m, na1)) if na1 else None
    d0, db = panels.up(A0, t), panels.up(B, t)
    d1 = panels.up(A1, t) if na1 else None
    na = t + na1
    out = np.zeros((na, t), order="F")
    panels.check(panels.L.preAlps_hip_panel_gram(C.byref(d0), C.byref(d1) if na1 else None, C.byref(db), _pd(out), na),
                 "gram")
    ref = (np.hstack([A0, A1]) if na1 else A0).T @ B
    np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("m", [7, 4099])
@pytest.mark.parametrize("t,na1,nc", [(2, 2, 2), (4, 4, 4), (4, 0, 4), (4, 4, 3), (8, 8, 8), (8, 5, 6), (8, 0, 8),
                                      (16, 16, 16), (16, 0, 16), (12, 9, 12)])
def test_update_z(panels, m, t, na1, nc):
    rng = np.random.default_rng(m + t + 5 * na1 + nc)
    Z, V0 = rng.standard_normal((m, nc)), rng.standard_normal((m, t))
    V1 = rng.standard_normal((m, na1)) if na1 else None
    na = t + na1
    beta = np.asfortranarray(rng.standard_normal((na, nc)))
    dz, d0 = panels.up(Z, t), panels.up(V0, t)
    d1 = panels.up(V1, t) if na1 else None
    panels.check(panels.L.preAlps_hip_panel_update(C.byref(dz), C.byref(d0), C.byref(d1) if na1 else None,
                                                  _pd(beta), na), "update")
    ref = Z - (np.hstack([V0, V1]) if na1 else V0) @ beta
    np.testing.assert_allclose(panels.down(dz, t), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("m", [5, 10007])
@pytest.mark.parametrize("t,nc", [(1, 1), (2, 2), (4, 4), (3, 4), (8, 8), (6, 8), (16, 16), (11, 16), (12, 12)])
def test_trsm_update(panels, m, t, nc):
    """t = current block size (columns of P, AP), nc = enlarging factor (columns of X, R)."""
    T = nc
    rng = np.random.default_rng(m + 17 * t + nc)
    P, AP = rng.standard_normal((m, t)), rng.standard_normal((m, t))
    X, R = rng.standard_normal((m, nc)), rng.standard_normal((m, nc))
    U = np.asfortranarray(np.triu(rng.standard_normal((t, t))) + 4.0 * np.eye(t))
    alpha = np.asfortranarray(rng.standard_normal((t, nc)))
    dp, dap, dx, dr = panels.up(P, T), panels.up(AP, T), panels.up(X, T), panels.up(R, T)
    res2 = C.c_double()
    panels.check(panels.L.preAlps_hip_panel_trsm_update(C.byref(dp), C.byref(dap), C.byref(dx), C.byref(dr),
                                                       _pd(U), _pd(alpha), C.byref(res2)), "trsm_update")
    Ui = np.linalg.inv(U)
    Pn, APn = P @ Ui, AP @ Ui
    Xn, Rn = X + Pn @ alpha, R - APn @ alpha
    for got, ref in ((panels.down(dp, T), Pn), (panels.down(dap, T), APn), (panels.down(dx, T), Xn),
                     (panels.down(dr, T), Rn)):
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-11 * np.abs(ref).max())
    assert abs(res2.value - (Rn ** 2).sum()) <= 1e-11 * (Rn ** 2).sum()


@pytest.mark.parametrize("m", [7, 30011])
@pytest.mark.parametrize("n,t", [(2, 2), (4, 4), (4, 3), (3, 1), (8, 8), (8, 5), (5, 5), (16, 16), (16, 9), (12, 0)])
def test_permute_solve(panels, m, n, t):
    """BF-Omin's copy + dlapmt + dtrsm (ecg.c:358-393) in one kernel: against numpy, and bit for bit against the
    three kernels it replaces; the columns behind the rank keep the permuted copy."""
    rng = np.random.default_rng(m + 13 * n + t)
    Z, P0 = rng.standard_normal((m, n)), rng.standard_normal((m, n))
    piv = rng.permutation(n).astype(np.int32)
    U = np.asfortranarray(np.triu(rng.standard_normal((t, t))) + 3.0 * np.eye(t)) if t else np.zeros((1, 1))
    outs = []
    for one_pass in (1, 0):
        dz, dp = panels.up(Z, n), panels.up(P0, n)
        panels.check(panels.L.preAlps_hip_panel_permute_solve(C.byref(dz), C.byref(dp), piv.ctypes.data_as(C.POINTER(C.c_int)),
                                                             t, _pd(U), one_pass), "permute_solve")
        outs.append(panels.down(dp, n))
        np.testing.assert_array_equal(panels.down(dz, n), Z)
    ref = Z[:, piv].copy()
    if t:
        ref[:, :t] = ref[:, :t] @ np.linalg.inv(U)
    np.testing.assert_allclose(outs[0], ref, rtol=1e-11, atol=1e-11 * np.abs(ref).max())
    np.testing.assert_array_equal(outs[0], outs[1])


def test_gram_finish_refusal_is_reported_and_harmless(panels):
    """pa_k_gram_finish refuses a [W ; G^T] request whose leading dimension is not t + T on the host, before the
    finishing launch: return code 1, the reason in pa_rt_error(), and the same buffers serve a valid call after it."""
    L = panels.L
    m, t = 64, 4
    L.pa_rt_error.restype = C.c_char_p
    L.pa_rt_malloc.restype = C.c_void_p
    L.pa_rt_malloc.argtypes = [C.c_size_t]
    L.pa_rt_free.argtypes = [C.c_void_p]
    L.pa_rt_free.restype = None
    L.pa_rt_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.pa_rt_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.pa_rt_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    vp, ci = C.c_void_p, C.c_int
    L.pa_k_gram.argtypes = [ci, ci, vp, vp, vp, vp, C.POINTER(ci)]
    L.pa_k_gram_finish.argtypes = [ci, ci, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, ci, vp, vp, vp]
    rng = np.random.default_rng(64 + t)
    A0, A1 = rng.standard_normal((m, t)), rng.standard_normal((m, t))      # (row-interleaved panels of stride t)
    bufs = []

    def dev(nbytes, src=None):
        d = L.pa_rt_malloc(nbytes)
        assert d
        bufs.append(d)
        panels.check(L.pa_rt_memset(d, 0, nbytes), "memset")
        if src is not None:
            panels.check(L.pa_rt_h2d(d, src.ctypes.data, src.nbytes), "h2d")
        return d

    def host(d, shape):
        h = np.zeros(shape, order="F")
        panels.check(L.pa_rt_d2h(h.ctypes.data, d, h.nbytes), "d2h")
        return h

    try:
        d0, d1 = dev(A0.nbytes, A0), dev(A1.nbytes, A1)
        part = dev(L.pa_gram_max_blocks() * 2 * t * t * 8)
        out, mu, alpha, info = dev(2 * t * t * 8), dev(t * t * 8), dev(t * t * 8), dev(8)
        nblk = ci(0)
        panels.check(L.pa_k_gram(m, t, d0, d1, d0, part, C.byref(nblk)), "gram")
        assert nblk.value >= 1
        rc = L.pa_k_gram_finish(m, t, d0, d1, d0, part, t, t, t, out, 2 * t + 1, t, t, mu, alpha, info)
        assert rc == 1
        assert "layout expected" in L.pa_rt_error().decode()
        assert L.pa_k_gram_finish(m, t, d0, d1, d0, part, t, t, t, out, 2 * t, t, t, mu, alpha, info) == 0
        panels.check(L.preAlps_hip_sync(), "sync")
        ref = np.hstack([A0, A1]).T @ A0                      # [W ; G^T], W = A0^T A0
        np.testing.assert_allclose(host(out, (2 * t, t)), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        U = np.linalg.cholesky(ref[:t]).T
        ref_alpha = np.linalg.solve(U.T, ref[t:].T)
        status = np.zeros(2, dtype=np.int32)
        panels.check(L.pa_rt_d2h(status.ctypes.data, info, 8), "d2h")
        assert status[0] == 0
        np.testing.assert_allclose(np.triu(host(mu, (t, t))), U, rtol=1e-11, atol=1e-11 * np.abs(U).max())
        np.testing.assert_allclose(host(alpha, (t, t)), ref_alpha, rtol=1e-11, atol=1e-11 * np.abs(ref_alpha).max())
    finally:
        for d in bufs:
            L.pa_rt_free(d)


# ---------------------------------------------------------------------------------------------------------------
# The paths the plain calls above do not take: the factor and alpha formed inside k_trsm_update (gram != NULL), the
# lazy coefficients of k_update_z, Z^T Z as its by-product, the packing of the send rows.  Through the pa_k_*
# launchers on raw device buffers (dense_dev.py), against dense_ref.py's longdouble references within their derived
# bounds (test_dense_ref_cpu.py); every test prints its worst ratio to the bound (pytest -s).
import dense_ref as D
from dense_dev import Dev


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("m", [5, 10007])
@pytest.mark.parametrize("ts,t", [(2, 2), (4, 3), (4, 4), (8, 7), (8, 8), (16, 15), (16, 16)])
def test_trsm_update_from_gram(dev, m, ts, t, keep):
    """gram = [W ; G^T] on the device: workgroup 0 writes U = chol(W) and alpha = U^-T G (backward error), every row
    is updated with them; with ukeep P and AP stay raw and the factor is kept."""
    import os
    assert "PREALPS_TRSM_MFMA" not in os.environ
    nc = t
    rng = np.random.default_rng(m + 17 * t + ts + keep)
    P, AP, X, R = (D.panel(rng, m, ts) for _ in range(4))
    A = rng.standard_normal((4 * t, t))
    W, G = A.T @ A, rng.standard_normal((t, nc))
    dP, dAP, dX, dR = (dev.up(a) for a in (P, AP, X, R))
    dgram = dev.upf(np.vstack([W, G.T]))
    dU, dalpha, dinfo, dkeep = dev.zeros(t * t * 8), dev.zeros(t * nc * 8), dev.up(np.array([4, 0], dtype=np.int32)), dev.zeros(t * t * 8)
    drtr = dev.zeros(512 * ts * 8)
    nblk = C.c_int(0)
    rc = dev.L.pa_k_trsm_update(m, ts, t, nc, dU, dalpha, dP, dAP, dX, dR, drtr, C.byref(nblk), 0, None, dinfo, None,
                                dgram, dkeep if keep else None)
    assert rc == 0, dev.error()
    assert dev.down(dinfo, (2,), np.int32)[0] == 0
    Ufull, alpha = dev.downf(dU, t, t), dev.downf(dalpha, t, nc)
    U = np.triu(Ufull)
    assert np.all(np.diag(U) > 0)
    zero = np.zeros((t, t))
    r = max(D.chol_backward(U, W, zero, t), D.alpha_backward(U, alpha, G, np.zeros((t, nc)), t))
    ref = D.trsm_update(P, AP, X, R, U, alpha, t, nc)
    bnd = D.trsm_update_bound(P, AP, X, R, U, alpha, t, nc, ts >= 8)
    got = [dev.down(d, (m, ts)) for d in (dP, dAP, dX, dR)]
    if keep:
        assert got[0].tobytes() == P.tobytes() and got[1].tobytes() == AP.tobytes()
        assert dev.downf(dkeep, t, t).tobytes() == Ufull.tobytes()
        r = max(r, D.ratio(got[2], ref[2], bnd[2]), D.ratio(got[3], ref[3], bnd[3]))
    else:
        r = max([r] + [D.ratio(g, rf, b) for g, rf, b in zip(got, ref, bnd)])
    print("trsm_update from gram m=%d ts=%d t=%d keep=%d: worst ratio %.3g" % (m, ts, t, keep, r))
    assert r <= 1.0


def _lazy_cases():
    for ts in (2, 4, 8, 16):
        for t in sorted({1, ts - 1, ts}):
            for a_hi in (0, t):
                yield ts, t, a_hi


@pytest.mark.parametrize("m", [7, 4099])
@pytest.mark.parametrize("ts,t,a_hi", list(_lazy_cases()))
def test_update_z_lazy(dev, m, ts, t, a_hi):
    """ucur / uprev given: Z' = Z Ui - V0 Ui (Ui^T G1 Ui) - V1 Up (Up^T G2 Ui) from the raw panels and Gram blocks."""
    rng = np.random.default_rng(m + 100 * ts + 10 * t + a_hi)
    Z, V0, V1 = D.panel(rng, m, ts), D.panel(rng, m, ts), D.panel(rng, m, ts)
    U, Up = D.factor(rng, t), D.factor(rng, t)
    beta = rng.standard_normal((t + a_hi, t))
    ldb = t + a_hi + 1
    dZ, dV0, dV1 = dev.up(Z), dev.up(V0), dev.up(V1)
    dbeta, dU, dUp = dev.upf(beta, ldb), dev.upf(U), dev.upf(Up)

    def call(nc):
        return dev.L.pa_k_update_z(m, ts, t, a_hi, nc, dbeta, ldb, dV0, dV1 if a_hi else None, dZ, None, None, dU, dUp,
                                   None, 0, None)

    if t > 1:
        assert call(t - 1) == 1
        assert "square blocks" in dev.error()
        assert dev.down(dZ, (m, ts)).tobytes() == Z.tobytes()
    assert call(t) == 0, dev.error()
    V1r = V1 if a_hi else None
    r = D.ratio(dev.down(dZ, (m, ts)), D.lazy_update_z(Z, V0, V1r, U, Up, beta, t),
                D.lazy_update_z_bound(Z, V0, V1r, U, Up, beta, t))
    for d, a in ((dV0, V0), (dV1, V1)):
        assert dev.down(d, (m, ts)).tobytes() == a.tobytes()
    print("update_z lazy m=%d ts=%d t=%d a_hi=%d: ratio %.3g" % (m, ts, t, a_hi, r))
    assert r <= 1.0


@pytest.mark.parametrize("m", [7, 4099])
@pytest.mark.parametrize("ts", [8, 16])
@pytest.mark.parametrize("less", [3, 0])
def test_update_z_leaves_ztz(dev, m, ts, less):
    """zz_part (8 / 16 columns, not lazy): one ts x ts block of Z'^T Z' per workgroup, summed by pa_k_finish."""
    zc = ts - less
    rng = np.random.default_rng(m + ts + less)
    Z, V0, V1 = D.panel(rng, m, ts), D.panel(rng, m, ts), D.panel(rng, m, ts)
    beta = rng.standard_normal((2 * ts, ts))
    dZ, dV0, dV1, dbeta = dev.up(Z), dev.up(V0), dev.up(V1), dev.upf(beta)
    dzz = dev.zeros(dev.L.pa_gram_max_blocks() * 2 * ts * ts * 8)      # (a Gram buffer: pa_k_finish's shares lie behind the blocks)
    dout = dev.zeros(zc * zc * 8)
    nblk = C.c_int(-1)
    rc = dev.L.pa_k_update_z(m, ts, ts, ts, ts, dbeta, 2 * ts, dV0, dV1, dZ, None, None, None, None, dzz, zc, C.byref(nblk))
    assert rc == 0, dev.error()
    assert nblk.value == min(2048, -(-m // 1024))
    assert dev.L.pa_k_finish(dzz, nblk.value, 1, ts, zc, 0, zc, dout, zc) == 0, dev.error()
    V = np.hstack([V0, V1])
    Zn = D.update_z(Z, V, beta, ts)
    Za, cz = D.update_z_abs(Z, V, beta, ts)
    r = D.ratio(dev.down(dZ, (m, ts)), Zn, (cz + D.SPARE) * D.UNIT * Za)
    r2 = D.ratio(dev.downf(dout, zc, zc), D.gram(Zn[:, :zc], Zn[:, :zc]),
                 D.gram_bound(Za[:, :zc], Za[:, :zc], c_in=2 * cz + D.SPARE))
    print("update_z with Z^T Z m=%d ts=%d cols=%d: Z %.3g, Z^T Z %.3g" % (m, ts, zc, r, r2))
    assert max(r, r2) <= 1.0


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("m", [7, 4099])
@pytest.mark.parametrize("ts", [2, 4])
def test_update_z_packs_the_send_rows(dev, m, ts, lazy):
    """pa_k_update_z_pack: the next update also writes the rows the neighbours need into the send buffer -- rows in
    no, one and three slots -- and only the next one."""
    t = ts
    rng = np.random.default_rng(m + ts + lazy)
    Z, V0, V1 = D.panel(rng, m, ts), D.panel(rng, m, ts), D.panel(rng, m, ts)
    U, Up = D.factor(rng, t), D.factor(rng, t)
    beta = rng.standard_normal((2 * t, t))
    cnt = rng.choice([0, 1, 3], size=m)
    cnt[:3] = [0, 1, 3]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    nslot = int(off[-1])
    slot = rng.permutation(nslot + 5)[:nslot].astype(np.int32)         # (distinct; five slots nobody writes)
    dZ, dV0, dV1, dbeta = dev.up(Z), dev.up(V0), dev.up(V1), dev.upf(beta)
    dU, dUp = dev.upf(U), dev.upf(Up)
    doff, dslot, dsend = dev.up(off), dev.up(slot), dev.zeros((nslot + 5) * ts * 8)

    def update():
        return dev.L.pa_k_update_z(m, ts, t, t, t, dbeta, 2 * t, dV0, dV1, dZ, None, None, dU if lazy else None,
                                   dUp if lazy else None, None, 0, None)

    assert dev.L.pa_k_update_z_pack(8, doff, dslot, dsend) == 0
    assert dev.L.pa_k_update_z_pack(ts, doff, dslot, dsend) == 1
    assert update() == 0, dev.error()
    Zn, send = dev.down(dZ, (m, ts)), dev.down(dsend, (nslot + 5, ts))
    want = np.zeros_like(send)
    for row in range(m):
        want[slot[off[row]:off[row + 1]]] = Zn[row]
    assert send.tobytes() == want.tobytes()
    ref = D.lazy_update_z(Z, V0, V1, U, Up, beta, t) if lazy else D.update_z(Z, np.hstack([V0, V1]), beta, t)
    Za, cz = D.update_z_abs(Z, np.hstack([V0, V1]), beta, t)
    bnd = D.lazy_update_z_bound(Z, V0, V1, U, Up, beta, t) if lazy else (cz + D.SPARE) * D.UNIT * Za
    assert D.ratio(Zn, ref, bnd) <= 1.0
    assert update() == 0, dev.error()                                  # the one-shot is spent
    assert dev.down(dsend, (nslot + 5, ts)).tobytes() == send.tobytes()
    assert dev.down(dZ, (m, ts)).tobytes() != Zn.tobytes()
