"""What finishes a Gram product, by itself: the sums of partial blocks by 64 workgroups and a ticket (k_finish32, its
pair and its form with the residual norm riding along), the Cholesky factor and alpha formed behind them
(potrf_alpha_wg) with the status of a failed factorisation, and the three dispatch branches of
pa_k_gram_finish_trace / the factoring form of pa_k_gram_finish.

Sums are held to the bounds of dense_ref.py (n 2^-53 sum |term| for a sum of n terms in whatever order); factors and
alpha to their backward error, mu^T mu = W and mu^T alpha = G, never to a reference factor.  A failed factorisation is
a status the kernel reports (info = the pivot's number); nothing here faults.  Every test prints its worst ratio to the
bound (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import dense_ref as D
from dense_dev import Dev

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def gram_parts(rng, nblk, t, T, rows=8):
    """(nblk, 32) partial blocks whose sum starts with a [W ; G^T] of (t + T) x t, W = sum A_b^T A_b (SPD), column
    major with leading dimension t + T as potrf_alpha_wg reads it; normals behind it."""
    parts = rng.standard_normal((nblk, 32))
    if t:
        A, B = rng.standard_normal((nblk, rows, t)), rng.standard_normal((nblk, rows, T))
        M = np.einsum("bki,bkj->bij", np.concatenate([A, B], axis=2), A)          # (nblk, t + T, t)
        parts[:, :(t + T) * t] = M.transpose(0, 2, 1).reshape(nblk, -1)
    return parts


def wg_of(vec, t, T):
    """W (t x t) and G (t x T) of a 32-vector that starts with the column-major [W ; G^T]."""
    M = np.asarray(vec)[:(t + T) * t].reshape(t, t + T).T
    return M[:t], M[t:].T


def check_factor(dev, dmu, dalpha, dinfo, t, T, ref, bnd):
    """Backward-error ratios of mu and alpha against the reference sum `ref` (32-vector) with its bound."""
    W, G = wg_of(ref, t, T)
    Wb, Gb = wg_of(bnd, t, T)
    mu, alpha = dev.downf(dmu, t, t), dev.downf(dalpha, t, T)
    assert dev.down(dinfo, (2,), np.int32)[0] == 0
    assert np.all(np.diag(mu) > 0)
    return max(D.chol_backward(mu, W, Wb, t), D.alpha_backward(mu, alpha, G, Gb, t))


def ticket(dev, dscr):
    nsh = dev.L.pa_finish32_scratch_blocks() - 1
    return int(dev.down(dscr, ((nsh + 1) * 32,))[nsh * 32:].view(np.uint32)[0])


@pytest.mark.parametrize("nblk", [1, 63, 64, 65, 4174, 8193])
@pytest.mark.parametrize("t", [0, 1, 2, 3, 4])
def test_finish32(dev, nblk, t):
    """Two calls in a row on one scratch, different partials: the sum, the factor and alpha behind it, the ticket."""
    assert dev.L.pa_finish32_scratch_blocks() == 65
    rng = np.random.default_rng(10 * nblk + t)
    dscr = dev.zeros(dev.L.pa_finish32_scratch_blocks() * 32 * 8)
    dout, dmu, dalpha, dinfo = dev.zeros(32 * 8), dev.zeros(16 * 8), dev.zeros(16 * 8), dev.zeros(8)
    worst = 0.0
    for call in range(2):
        parts = gram_parts(rng, nblk, t, t)
        dparts = dev.up(parts)
        dev.put(dinfo, np.array([7, 0], dtype=np.int32))
        rc = dev.L.pa_k_finish32(dparts, nblk, dscr, t, t, dout, dmu if t else None, dalpha if t else None,
                                 dinfo if t else None)
        assert rc == 0, dev.error()
        ref, bnd = D.sum_blocks(parts), D.sum_blocks_bound(parts)
        worst = max(worst, D.ratio(dev.down(dout, (32,)), ref, bnd))
        if t:
            worst = max(worst, check_factor(dev, dmu, dalpha, dinfo, t, t, ref, bnd))
        assert ticket(dev, dscr) == 0
    print("finish32 nblk=%d t=%d: worst ratio %.3g" % (nblk, t, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("na,nb", [(1, 8193), (4174, 65)])
def test_finish32_pair(dev, na, nb):
    """One launch for two sums: the bytes of two pa_k_finish32 calls."""
    t = 4
    rng = np.random.default_rng(na + nb)
    pa, pb = gram_parts(rng, na, t, t), gram_parts(rng, nb, 0, 0)
    dpa, dpb = dev.up(pa), dev.up(pb)
    nscr = dev.L.pa_finish32_scratch_blocks() * 32 * 8
    outs = []
    for pair in (1, 0):
        dsa, dsb = dev.zeros(nscr), dev.zeros(nscr)
        doa, dob, dmu, dalpha, dinfo = dev.zeros(32 * 8), dev.zeros(32 * 8), dev.zeros(16 * 8), dev.zeros(16 * 8), dev.zeros(8)
        if pair:
            assert dev.L.pa_k_finish32_pair(dpa, na, dsa, t, t, doa, dmu, dalpha, dinfo, dpb, nb, dsb, dob) == 0, dev.error()
        else:
            assert dev.L.pa_k_finish32(dpa, na, dsa, t, t, doa, dmu, dalpha, dinfo) == 0, dev.error()
            assert dev.L.pa_k_finish32(dpb, nb, dsb, 0, 0, dob, None, None, None) == 0, dev.error()
        outs.append([dev.down(d, (n,)).tobytes() for d, n in ((doa, 32), (dmu, 16), (dalpha, 16), (dob, 32))])
        assert dev.down(dinfo, (2,), np.int32)[0] == 0
        assert ticket(dev, dsa) == 0 and ticket(dev, dsb) == 0
    assert outs[0] == outs[1]
    ref, bnd = D.sum_blocks(pa), D.sum_blocks_bound(pa)
    assert D.ratio(np.frombuffer(outs[0][0]), ref, bnd) <= 1.0
    assert D.ratio(np.frombuffer(outs[0][3]), D.sum_blocks(pb), D.sum_blocks_bound(pb)) <= 1.0


@pytest.mark.parametrize("rtr_nblk", [1, 255, 256, 257, 512])
@pytest.mark.parametrize("nc", [1, 3, 4])
def test_finish32_trace(dev, rtr_nblk, nc):
    ts, nblk = 4, 65
    rng = np.random.default_rng(rtr_nblk + nc)
    parts, rtr = gram_parts(rng, nblk, 0, 0), rng.standard_normal((rtr_nblk, ts)) ** 2
    dparts, drtr = dev.up(parts), dev.up(rtr)
    dscr = dev.zeros(dev.L.pa_finish32_scratch_blocks() * 32 * 8)
    dout, dres, dinfo = dev.zeros(32 * 8), dev.zeros(16), dev.up(np.array([5, 0], dtype=np.int32))
    assert dev.L.pa_k_finish32_trace(dparts, nblk, dscr, dout, drtr, rtr_nblk, ts, nc, dres, dinfo) == 0, dev.error()
    res2 = dev.down(dres, (2,))
    terms = rtr[:, :nc].reshape(-1, 1)
    r = max(D.ratio(dev.down(dout, (32,)), D.sum_blocks(parts), D.sum_blocks_bound(parts)),
            D.ratio(res2[:1], D.sum_blocks(terms), D.sum_blocks_bound(terms)))
    print("finish32_trace rtr_nblk=%d nc=%d: worst ratio %.3g" % (rtr_nblk, nc, r))
    assert r <= 1.0
    assert res2[1] == 5.0
    assert ticket(dev, dscr) == 0


@pytest.mark.parametrize("through", ["potrf_alpha", "finish32"])
@pytest.mark.parametrize("j", [0, 2, 3, "nan"])
def test_failed_factorisation_is_reported(dev, through, j):
    """W built SPD, then W[j, j] lowered so that pivot j is about -1 (or W[0, 0] = NaN): info = j + 1, the rows of mu
    above the pivot are a factor of the leading block, the pivot itself is stored and is not positive."""
    t = T = 4
    nblk = 65
    rng = np.random.default_rng(11)
    parts = gram_parts(rng, nblk, t, T)
    W = wg_of(parts.sum(axis=0), t, T)[0]
    Uf = np.linalg.cholesky(W).T
    jj = 0 if j == "nan" else j
    parts[0, jj + (t + T) * jj] = np.nan if j == "nan" else parts[0, jj + (t + T) * jj] - (Uf[jj, jj] ** 2 + 1.0)
    dmu, dalpha, dinfo = dev.zeros(16 * 8), dev.zeros(16 * 8), dev.zeros(8)
    if through == "finish32":
        dparts, dout = dev.up(parts), dev.zeros(32 * 8)
        dscr = dev.zeros(dev.L.pa_finish32_scratch_blocks() * 32 * 8)
        assert dev.L.pa_k_finish32(dparts, nblk, dscr, t, T, dout, dmu, dalpha, dinfo) == 0, dev.error()
        ref, bnd = D.sum_blocks(parts), D.sum_blocks_bound(parts)
        assert ticket(dev, dscr) == 0
    else:
        buf = parts.sum(axis=0)
        dbuf = dev.up(buf)
        assert dev.L.pa_k_potrf_alpha(dbuf, t, T, dmu, dalpha, dinfo) == 0, dev.error()
        ref, bnd = D.ld(buf), np.zeros(32)
    assert dev.down(dinfo, (2,), np.int32)[0] == jj + 1
    mu = dev.downf(dmu, t, t)
    assert not mu[jj, jj] > 0
    r = D.chol_backward(mu, wg_of(ref, t, T)[0], wg_of(bnd, t, T)[0], jj)
    print("failed pivot %s through %s: leading block ratio %.3g, pivot %g" % (j, through, r, mu[jj, jj]))
    assert r <= 1.0
    if j != "nan":
        assert -1.5 < mu[jj, jj] < -0.5


def gram_inputs(m, ts, a_lo, a_hi, nb):
    rng = np.random.default_rng(m + 100 * ts + 10 * a_lo + a_hi + nb)
    A0, A1, B = D.panel(rng, m, ts), D.panel(rng, m, ts), D.panel(rng, m, ts)
    A = np.hstack([A0[:, :a_lo], A1[:, :a_hi]])
    return A0, A1, B, A


WIDE = [(8, 8, 8, 8), (8, 5, 3, 6), (8, 8, 0, 8), (16, 16, 16, 16), (16, 12, 7, 12), (16, 16, 0, 16)]
NARROW = [(2, 2, 2, 2), (4, 4, 4, 4), (4, 3, 2, 3), (4, 4, 0, 4), (2, 1, 0, 1)]
NONE = [(4, 0, 0, 0), (8, 0, 0, 0)]


@pytest.mark.parametrize("m", [1, 1000, 40961])
@pytest.mark.parametrize("ts,a_lo,a_hi,nb", WIDE + NARROW + NONE)
def test_gram_finish_trace(dev, m, ts, a_lo, a_hi, nb):
    """The three branches: wide blocks (several workgroups, the last adds the norm), a block one workgroup sums with
    the norm behind it, and no block at all (the norm alone)."""
    A0, A1, B, A = gram_inputs(m, ts, a_lo, a_hi, nb)
    rtr_nblk, nc = 257, min(3, ts)
    rtr = np.random.default_rng(m + ts).standard_normal((rtr_nblk, ts)) ** 2
    d0, d1, db, drtr = dev.up(A0), dev.up(A1), dev.up(B), dev.up(rtr)
    dpart = dev.zeros(dev.L.pa_gram_max_blocks() * 2 * ts * ts * 8)
    na = a_lo + a_hi
    dout, dres, dinfo = dev.zeros(max(na * nb, 1) * 8), dev.zeros(16), dev.up(np.array([2, 0], dtype=np.int32))
    rc = dev.L.pa_k_gram_finish_trace(m, ts, d0, d1 if a_hi else None, db, dpart, a_lo, a_hi, nb, dout, max(na, 1),
                                      drtr, rtr_nblk, nc, dres, dinfo)
    assert rc == 0, dev.error()
    res2 = dev.down(dres, (2,))
    terms = rtr[:, :nc].reshape(-1, 1)
    r = D.ratio(res2[:1], D.sum_blocks(terms), D.sum_blocks_bound(terms))
    if na * nb:
        r = max(r, D.ratio(dev.downf(dout, na, nb), D.gram(A, B[:, :nb]), D.gram_bound(A, B[:, :nb])))
    print("gram_finish_trace m=%d ts=%d %d+%d x %d: worst ratio %.3g" % (m, ts, a_lo, a_hi, nb, r))
    assert r <= 1.0
    assert res2[1] == 2.0


@pytest.mark.parametrize("m", [1000, 40961])
@pytest.mark.parametrize("ts,t", [(2, 2), (4, 3), (4, 4), (8, 7), (8, 8), (16, 15), (16, 16)])
def test_gram_finish_factors(dev, m, ts, t):
    """pa_k_gram_finish with t = T > 0: [W ; G^T] = [A0 | A1]^T A0, its factor and alpha, in one call."""
    A0, A1, _, A = gram_inputs(m, ts, t, t, t)
    d0, d1 = dev.up(A0), dev.up(A1)
    dpart = dev.zeros(dev.L.pa_gram_max_blocks() * 2 * ts * ts * 8)
    dout, dmu, dalpha, dinfo = dev.zeros(2 * t * t * 8), dev.zeros(t * t * 8), dev.zeros(t * t * 8), dev.up(np.array([9, 0], dtype=np.int32))
    rc = dev.L.pa_k_gram_finish(m, ts, d0, d1, d0, dpart, t, t, t, dout, 2 * t, t, t, dmu, dalpha, dinfo)
    assert rc == 0, dev.error()
    ref, bnd = D.gram(A, A0[:, :t]), D.gram_bound(A, A0[:, :t])
    r = D.ratio(dev.downf(dout, 2 * t, t), ref, bnd)
    assert dev.down(dinfo, (2,), np.int32)[0] == 0
    mu, alpha = dev.downf(dmu, t, t), dev.downf(dalpha, t, t)
    assert np.all(np.diag(mu) > 0)
    r = max(r, D.chol_backward(mu, ref[:t], bnd[:t], t), D.alpha_backward(mu, alpha, ref[t:].T, bnd[t:].T, t))
    print("gram_finish m=%d ts=%d t=%d: worst ratio %.3g" % (m, ts, t, r))
    assert r <= 1.0
