"""The row pass of the default configuration by itself: k_update_xrz<4, EVERY | SKIP | BOTH>, k_flush_x and
k_trace_finish through their launchers (pa_k_update_xrz_mode, pa_k_flush_x, pa_k_trace_finish), against the longdouble
reference of dense_ref.py within its derived bound (test_dense_ref_cpu.py shows the bound sound and sharp).

Single pass: every t of a 4-wide panel, row counts around one workgroup (256 rows), around its two rows per lane
(513) and 262147 = 513 workgroups' worth of rows against the cap of 512, so that some lanes make a ragged third pass;
beta with and without padding in its leading dimension.  Deferred X: two iterations with the panels rotated as
ecg_loops.c rotates them (P -> P_prev, Z -> P, the kept factor -> uprev), at row counts on both sides of the 16 MiB
switch to nontemporal X.  The refusals of the launcher.  Every test prints its worst ratio to the bound (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_ref as D
from dense_dev import Dev

pytestmark = pytest.mark.gpu
TS = 4
EVERY, SKIP, BOTH = 0, 1, 2


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


@functools.lru_cache(maxsize=2)
def panels_of(m, n):
    """n random panels of m rows, the same for every case of this row count."""
    rng = np.random.default_rng(m)
    out = tuple(D.panel(rng, m, TS) for _ in range(n))
    for a in out:
        a.setflags(write=False)
    return out


def small(rng, t):
    """U, alpha, beta = [G1 ; G2] of one iteration."""
    return D.factor(rng, t), rng.standard_normal((t, t)), rng.standard_normal((2 * t, t))


def xrz(dev, m, t, dU, da, dP, dAP, dPp, dX, dR, dZ, drtr, dkeep, dbeta, ldb, duprev, mode, dakeep, ts=TS):
    nblk = C.c_int(-1)
    rc = dev.L.pa_k_update_xrz_mode(m, ts, t, dU, da, dP, dAP, dPp, dX, dR, dZ, drtr, C.byref(nblk), dkeep, dbeta, ldb,
                                    duprev, mode, dakeep)
    return rc, nblk.value


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 513, 262147])
@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_single_pass(dev, m, t, pad):
    P, AP, Pp, X, R, Z = panels_of(m, 6)
    rng = np.random.default_rng(100 * t + pad)
    U, alpha, beta = small(rng, t)
    Up = D.factor(rng, t)
    ldb = 2 * t + pad
    dP, dAP, dPp, dX, dR, dZ = (dev.up(a) for a in (P, AP, Pp, X, R, Z))
    dU, da, dbeta, dUp = dev.upf(U), dev.upf(alpha), dev.upf(beta, ldb), dev.upf(Up)
    dkeep, drtr = dev.zeros(16 * 8), dev.zeros(D.UPDATE_CAP * TS * 8)
    rc, nblk = xrz(dev, m, t, dU, da, dP, dAP, dPp, dX, dR, dZ, drtr, dkeep, dbeta, ldb, dUp, EVERY, None)
    assert rc == 0, dev.error()
    assert nblk == min(512, -(-m // 512))
    info = np.array([3, 0], dtype=np.int32)
    dinfo, dres = dev.up(info), dev.zeros(16)
    assert dev.L.pa_k_trace_finish(drtr, nblk, TS, TS, dres, dinfo, None) == 0, dev.error()
    ref = D.row_pass(P, AP, Pp, X, R, Z, U, alpha, beta, Up, t)
    bnd = D.row_pass_bound(P, AP, Pp, X, R, Z, U, alpha, beta, Up, t, D.passes(m, nblk))
    got = [dev.down(d, (m, TS)) for d in (dX, dR, dZ)]
    for d, a in ((dP, P), (dAP, AP), (dPp, Pp)):
        assert dev.down(d, (m, TS)).tobytes() == a.tobytes()
    assert dev.downf(dkeep, t, t).tobytes() == np.ascontiguousarray(U).tobytes()
    parts = dev.down(drtr, (nblk, TS))
    assert np.all(parts[:, t:] == 0)
    res2 = dev.down(dres, (2,))
    ratios = [D.ratio(g, r, b) for g, r, b in zip(got, ref[:3], bnd[:3])]
    ratios.append(D.ratio(D.ld(parts).sum(axis=0), ref[3], bnd[3]))
    ratios.append(D.ratio(res2[0], ref[3].sum(), D.trace_bound(P, AP, X, R, U, alpha, t, nblk, TS)))
    print("row pass m=%d t=%d ldb=%d: X %.3g R %.3g Z %.3g sums %.3g norm %.3g" % ((m, t, ldb) + tuple(ratios)))
    for c in range(t, TS):
        for g, a in zip(got, (X, R, Z)):
            assert g[:, c].tobytes() == np.ascontiguousarray(a[:, c]).tobytes()
    assert max(ratios) <= 1.0
    assert res2[1] == 3.0


@pytest.mark.parametrize("m", [257, 262147, 524287, 524288])
@pytest.mark.parametrize("t", [3, 4])
def test_deferred_x(dev, m, t):
    """EVERY, EVERY against SKIP, BOTH and against SKIP, flush: the same bytes, and the right ones."""
    P1, AP1, P0, X, R, Z1, AP2, Z2 = panels_of(m, 8)
    rng = np.random.default_rng(7 * t + 1)
    it = [small(rng, t), small(rng, t)]
    U0 = D.factor(rng, t)
    ldb = 2 * t
    worst = []

    def run(modes, flush=False):
        """Two passes (one when flush) in these X modes; what the device holds after each."""
        dP1, dAP1, dP0, dX, dR, dZ1, dAP2, dZ2 = (dev.up(a) for a in (P1, AP1, P0, X, R, Z1, AP2, Z2))
        duu = [dev.upf(U0), dev.zeros(16 * 8)]            # the kept factors: slot 0 holds U_prev of the first pass
        dak = [dev.zeros(16 * 8), dev.zeros(16 * 8)]
        drtr = dev.zeros(D.UPDATE_CAP * TS * 8)
        cur = 1
        rot = [(dP1, dAP1, dP0, dZ1), (dZ1, dAP2, dP1, dZ2)]      # (P, AP, P_prev, Z): Z of the first pass is P of the second
        states = []
        for k, mode in enumerate(modes):
            U, alpha, beta = it[k]
            dU, da, dbeta = dev.upf(U), dev.upf(alpha), dev.upf(beta)
            dP, dAP, dPp, dZ = rot[k]
            rc, _ = xrz(dev, m, t, dU, da, dP, dAP, dPp, dX, dR, dZ, drtr, duu[cur], dbeta, ldb, duu[1 - cur], mode,
                        dak[1 - cur] if mode == BOTH else dak[cur])
            assert rc == 0, dev.error()
            st = dict(X=dev.down(dX, (m, TS)), R=dev.down(dR, (m, TS)), Z=dev.down(dZ, (m, TS)),
                      akeep=dev.downf(dak[cur], t, t), ukeep=dev.downf(duu[cur], t, t))
            if flush:
                assert dev.L.pa_k_flush_x(m, TS, t, duu[cur], dak[cur], dP, dX) == 0, dev.error()
                st["Xflushed"] = dev.down(dX, (m, TS))
            states.append(st)
            cur = 1 - cur
        for d in dev.bufs[-(8 + 5 + 3 * len(modes)):]:
            dev.L.pa_rt_free(d)
        del dev.bufs[-(8 + 5 + 3 * len(modes)):]
        return states

    a = run((EVERY, EVERY))
    b = run((SKIP, BOTH))
    c = run((SKIP,), flush=True)
    # a skipping pass leaves X alone and keeps alpha
    assert b[0]["X"].tobytes() == X.tobytes()
    assert b[0]["akeep"].tobytes() == np.ascontiguousarray(it[0][1]).tobytes()
    assert b[0]["ukeep"].tobytes() == np.ascontiguousarray(it[0][0]).tobytes()
    for k in ("R", "Z"):
        assert b[0][k].tobytes() == a[0][k].tobytes()
    for k in ("X", "R", "Z"):
        assert b[1][k].tobytes() == a[1][k].tobytes(), k
    assert c[0]["Xflushed"].tobytes() == a[0]["X"].tobytes()
    # ... and the bytes are the right ones: each pass of EVERY, EVERY against the reference on what it was given
    U, alpha, beta = it[0]
    ref = D.row_pass(P1, AP1, P0, X, R, Z1, U, alpha, beta, U0, t)
    bnd = D.row_pass_bound(P1, AP1, P0, X, R, Z1, U, alpha, beta, U0, t)
    worst += [D.ratio(a[0][k], r, bb) for k, r, bb in zip("XRZ", ref, bnd)]
    worst.append(D.ratio(c[0]["Xflushed"], D.owed_x(X, P1, U, alpha, t), D.owed_x_bound(X, P1, U, alpha, t)))
    U2, alpha2, beta2 = it[1]
    ref = D.row_pass(a[0]["Z"], AP2, P1, a[0]["X"], a[0]["R"], Z2, U2, alpha2, beta2, U, t)
    bnd = D.row_pass_bound(a[0]["Z"], AP2, P1, a[0]["X"], a[0]["R"], Z2, U2, alpha2, beta2, U, t)
    worst += [D.ratio(a[1][k], r, bb) for k, r, bb in zip("XRZ", ref, bnd)]
    print("deferred X m=%d t=%d: worst ratio %.3g" % (m, t, max(worst)))
    assert max(worst) <= 1.0


def test_refusals(dev):
    m, t = 300, 4
    P, AP, Pp, X, R, Z = panels_of(m, 6)
    rng = np.random.default_rng(5)
    U, alpha, beta = small(rng, t)
    Up = D.factor(rng, t)
    # (panels of 8 columns' size, so that even a call that is not refused stays inside them)
    dP, dAP, dPp, dX, dR, dZ = (dev.up(a, extra=a.nbytes) for a in (P, AP, Pp, X, R, Z))
    dU, da, dbeta, dUp = dev.upf(U), dev.upf(alpha), dev.upf(beta), dev.upf(Up)
    dkeep, dak, drtr = dev.zeros(64 * 8), dev.zeros(64 * 8), dev.zeros(D.UPDATE_CAP * 16 * 8)

    def call(ts=TS, tt=t, ldb=2 * t, mode=EVERY, ak=None):
        return xrz(dev, m, tt, dU, da, dP, dAP, dPp, dX, dR, dZ, drtr, dkeep, dbeta, ldb, dUp, mode, ak, ts=ts)[0]

    for kw, text in ((dict(ts=8), "4-column panels"), (dict(tt=5, ldb=10), "4-column panels"),
                     (dict(ldb=2 * t - 1), "4-column panels"), (dict(mode=SKIP), "kept alpha")):
        assert call(**kw) == 1
        assert text in dev.error()
    for d, a in ((dX, X), (dR, R), (dZ, Z)):
        assert dev.down(d, (m, TS)).tobytes() == a.tobytes()
    assert call() == 0, dev.error()
    ref = D.row_pass(P, AP, Pp, X, R, Z, U, alpha, beta, Up, t)
    bnd = D.row_pass_bound(P, AP, Pp, X, R, Z, U, alpha, beta, Up, t)
    for d, r, b in zip((dX, dR, dZ), ref, bnd):
        assert D.ratio(dev.down(d, (m, TS)), r, b) <= 1.0
    assert call(mode=SKIP, ak=dak) == 0, dev.error()
