"""dense_ref.py's bounds are sound and sharp, without a GPU: for every reference function a float64 restatement of
the kernel's operations (numpy, the kernel's order of operations where the count depends on it) stays within the bound
-- worst ratio <= 1 -- and every seeded mistake applied to that restatement exceeds it -- worst ratio > 1.  So the
assertions of the GPU tests cannot fail for rounding and do fail for the mistakes a kernel can make: a row left out, a
second grid-stride pass left out, alpha transposed, the wrong factor, the Gram blocks swapped, a column too few, a
partial block dropped or added twice, a sign.  Every case prints its ratios (pytest -s)."""
import numpy as np
import pytest

import dense_ref as D

F = np.float64


# ----------------------------------------------------------------------------- the float64 restatements ----
def m_subst(P, U, t):
    """p <- p U^-1 along the rows, as trsm_update_row."""
    p = np.array(P, dtype=F)
    sd = 1.0 / np.diag(U)[:t]
    for j in range(t):
        s = P[:, j].copy()
        for k in range(j):
            s = s - p[:, k] * U[k, j]
        p[:, j] = s * sd[j]
    return p


def m_coeffs(U, Uprev, beta, t, a_hi, bug):
    Ui, Up = D.inv_upper(U[:t, :t], F), D.inv_upper(Uprev[:t, :t], F)
    G1, G2 = beta[:t, :t], (beta[t:2 * t, :t] if a_hi else np.zeros((t, t)))
    if bug == "swap_g":
        G1, G2 = G2, G1
    U1 = Up if bug == "uprev_for_u" else Ui
    C1 = U1 @ (U1.T @ (G1 @ Ui))
    C2 = Up @ (Up.T @ (G2 @ Ui))
    return Ui, C1, C2


def rows_left_out(m, bug):
    """The rows a mistake leaves as they were."""
    if bug == "last_row":
        return slice(m - 1, m)
    if bug == "second_pass":
        return slice(D.update_grid(m) * D.WG, m)
    return slice(0, 0)


def applies(bug, m, t, a_hi=1):
    if bug == "second_pass":
        return m > D.update_grid(m) * D.WG
    if bug == "alpha_T":
        return t >= 2
    if bug in ("swap_g", "z3_sign"):
        return a_hi > 0
    return True


def m_lazy_z(Z, V0, V1, U, Uprev, beta, t, bug=None):
    a_hi = 0 if V1 is None else t
    ta = t - 1 if bug == "inactive_col" else t
    Ui, C1, C2 = m_coeffs(U, Uprev, beta, t, a_hi, bug)
    out = Z.copy()
    act = Z[:, :t] @ Ui - V0[:, :t] @ C1
    if a_hi:
        act = act + (V1[:, :t] @ C2) * (1.0 if bug == "z3_sign" else -1.0)
    out[:, :ta] = act[:, :ta]
    keep = rows_left_out(Z.shape[0], bug)
    out[keep] = Z[keep]
    return out


def m_xr(P, AP, X, R, U, alpha, t, nc, bug=None, mfma=False):
    a = alpha[:t, :nc].T.copy() if bug == "alpha_T" else alpha[:t, :nc]
    Pn, APn = P.copy(), AP.copy()
    if mfma:        # k_trsm_update_mfma: Ui, then B = Ui alpha, products with the old tiles
        Ui = D.inv_upper(U[:t, :t], F)
        Pn[:, :t], APn[:, :t] = P[:, :t] @ Ui, AP[:, :t] @ Ui
        B = Ui @ a
        dx, dr = P[:, :t] @ B, AP[:, :t] @ B
    else:
        Pn[:, :t], APn[:, :t] = m_subst(P[:, :t], U, t), m_subst(AP[:, :t], U, t)
        dx, dr = Pn[:, :t] @ a, APn[:, :t] @ a
    na = nc - 1 if bug == "inactive_col" else nc
    Xn, Rn = X.copy(), R.copy()
    Xn[:, :na] = X[:, :na] + (-dx if bug == "x_minus" else dx)[:, :na]
    Rn[:, :na] = R[:, :na] - dr[:, :na]
    keep = rows_left_out(P.shape[0], bug)
    for new, old in ((Pn, P), (APn, AP), (Xn, X), (Rn, R)):
        new[keep] = old[keep]
    return Pn, APn, Xn, Rn


def m_colsum_partials(Rn, t, nblk):
    """block_sum_cols on r^2: a lane over its grid-stride rows, the wavefront's butterfly, the four wavefronts."""
    m, ts = Rn.shape
    npass = D.passes(m, nblk)
    sq = np.zeros((npass * nblk * D.WG, ts))
    sq[:m, :t] = Rn[:, :t] * Rn[:, :t]
    sq = sq.reshape(npass, nblk, 4, 64, ts)
    acc = np.zeros(sq.shape[1:])
    for p in range(npass):
        acc = acc + sq[p]
    n = 64
    while n > 1:
        acc = acc[:, :, :n // 2] + acc[:, :, n // 2:n]
        n //= 2
    acc = acc[:, :, 0]
    out = acc[:, 0]
    for w in range(1, 4):
        out = out + acc[:, w]
    return out                       # (nblk, ts)


def m_trace(parts, nc):
    """trace_finish_wg: a thread's blocks and columns one after the other, then the tree over 256 threads."""
    nblk = parts.shape[0]
    red = np.zeros(D.WG)
    for b in range(nblk):
        for c in range(nc):
            red[b % D.WG] = red[b % D.WG] + parts[b, c]
    n = D.WG
    while n > 1:
        red = red[:n // 2] + red[n // 2:n]
        n //= 2
    return red[0]


def m_sum(parts, bug=None):
    p = parts
    if bug == "drop_block":
        p = parts[:-1] if parts.shape[0] > 1 else parts * 0
    if bug == "double_block":
        p = np.concatenate([parts, parts[parts.shape[0] // 2:parts.shape[0] // 2 + 1]])
    return np.add.reduce(p, axis=0)


def m_chol_alpha(W, G, t):
    """dpotf2 'U' and the forward substitution with U^T, one entry after the other."""
    mu = np.zeros((t, t))
    for j in range(t):
        d = W[j, j]
        for k in range(j):
            d = d - mu[k, j] * mu[k, j]
        mu[j, j] = np.sqrt(d)
        for i in range(j + 1, t):
            s = W[j, i]
            for k in range(j):
                s = s - mu[k, j] * mu[k, i]
            mu[j, i] = s / mu[j, j]
    al = np.zeros_like(G)
    for i in range(t):
        s = G[i].copy()
        for k in range(i):
            s = s - mu[k, i] * al[k]
        al[i] = s / mu[i, i]
    return mu, al


def report(what, good, bad):
    print("%-46s f64 %.3g   mistakes %s" % (what, good, ", ".join("%s %.3g" % kv for kv in bad.items())))
    assert good <= 1.0, what
    for name, r in bad.items():
        assert r > 1.0, (what, name)


# ------------------------------------------------------------------------------------------------ tests ----
ROW_BUGS = ("last_row", "second_pass", "alpha_T", "uprev_for_u", "swap_g", "inactive_col", "x_minus", "z3_sign")


@pytest.mark.parametrize("m", [1, 255, 256, 257, 513, 4099])
@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_row_pass(m, t):
    ts = 4
    rng = np.random.default_rng(1000 * t + m)
    P, AP, Pp, X, R, Z = (D.panel(rng, m, ts) for _ in range(6))
    U, Up = D.factor(rng, t), D.factor(rng, t)
    alpha, beta = rng.standard_normal((t, t)), rng.standard_normal((2 * t, t))
    nblk = D.update_grid(m)
    assert nblk == min(512, -(-m // 512))
    ref = D.row_pass(P, AP, Pp, X, R, Z, U, alpha, beta, Up, t)
    bnd = D.row_pass_bound(P, AP, Pp, X, R, Z, U, alpha, beta, Up, t)
    for c in range(t, ts):
        assert ref[3][c] == 0 and np.array_equal(ref[0][:, c], X[:, c]) and np.array_equal(ref[2][:, c], Z[:, c])

    def worst(bug):
        _, _, Xn, Rn = m_xr(P, AP, X, R, U, alpha, t, t, bug)
        Zn = m_lazy_z(Z, P, Pp, U, Up, beta, t, bug)
        parts = m_colsum_partials(Rn, t, nblk)
        assert np.all(parts[:, t:] == 0)
        S = D.ld(parts).sum(axis=0)
        tr = D.ratio(m_trace(parts, ts), ref[3].sum(), D.trace_bound(P, AP, X, R, U, alpha, t, nblk, ts))
        return max(D.ratio(Xn, ref[0], bnd[0]), D.ratio(Rn, ref[1], bnd[1]), D.ratio(Zn, ref[2], bnd[2]),
                   D.ratio(S, ref[3], bnd[3]), tr)

    report("row_pass m=%d t=%d" % (m, t), worst(None), {b: worst(b) for b in ROW_BUGS if applies(b, m, t)})
    # the column sums alone: a workgroup's sums left out, or added twice
    parts = m_colsum_partials(m_xr(P, AP, X, R, U, alpha, t, t)[3], t, nblk)
    lim = bnd[3] + D.sum_blocks_bound(parts)
    bad = {b: D.ratio(m_sum(parts, b), ref[3], lim) for b in ("drop_block", "double_block")}
    report("row_pass column sums m=%d t=%d" % (m, t), D.ratio(m_sum(parts), ref[3], lim), bad)


@pytest.mark.parametrize("m", [257, 4099])
@pytest.mark.parametrize("t", [3, 4])
def test_owed_x(m, t):
    ts = 4
    rng = np.random.default_rng(77 * t + m)
    X, Pp = D.panel(rng, m, ts), D.panel(rng, m, ts)
    Up, ak = D.factor(rng, t), rng.standard_normal((t, t))
    ref, bnd = D.owed_x(X, Pp, Up, ak, t), D.owed_x_bound(X, Pp, Up, ak, t)

    def worst(bug):
        return D.ratio(m_xr(Pp, Pp, X, X, Up, ak, t, t, bug)[2], ref, bnd)

    bugs = ("last_row", "second_pass", "alpha_T", "inactive_col", "x_minus")
    report("owed_x m=%d t=%d" % (m, t), worst(None), {b: worst(b) for b in bugs if applies(b, m, t)})


def lazy_cases():
    for ts in (2, 4, 8, 16):
        for t in sorted({1, ts - 1, ts}):
            for a_hi in (0, t):
                yield ts, t, a_hi


@pytest.mark.parametrize("m", [7, 4099])
@pytest.mark.parametrize("ts,t,a_hi", list(lazy_cases()))
def test_lazy_update_z(m, ts, t, a_hi):
    rng = np.random.default_rng(m + 100 * ts + 10 * t + a_hi)
    Z, V0 = D.panel(rng, m, ts), D.panel(rng, m, ts)
    V1 = D.panel(rng, m, ts) if a_hi else None
    U, Up = D.factor(rng, t), D.factor(rng, t)
    beta = rng.standard_normal((t + a_hi, t))
    ref, bnd = D.lazy_update_z(Z, V0, V1, U, Up, beta, t), D.lazy_update_z_bound(Z, V0, V1, U, Up, beta, t)
    assert np.array_equal(ref[:, t:], Z[:, t:])

    def worst(bug):
        return D.ratio(m_lazy_z(Z, V0, V1, U, Up, beta, t, bug), ref, bnd)

    bugs = ("last_row", "second_pass", "uprev_for_u", "swap_g", "inactive_col", "z3_sign")
    report("lazy_update_z m=%d ts=%d t=%d a_hi=%d" % (m, ts, t, a_hi), worst(None),
           {b: worst(b) for b in bugs if applies(b, m, t, a_hi)})


@pytest.mark.parametrize("m", [5, 4099])
@pytest.mark.parametrize("ts,t", [(2, 2), (4, 3), (4, 4), (8, 7), (8, 8), (16, 15), (16, 16)])
def test_trsm_update(m, ts, t):
    nc = t
    rng = np.random.default_rng(m + 17 * t + ts)
    P, AP, X, R = (D.panel(rng, m, ts) for _ in range(4))
    U, alpha = D.factor(rng, t), rng.standard_normal((t, nc))
    ref = D.trsm_update(P, AP, X, R, U, alpha, t, nc)
    for mfma in ((False, True) if ts >= 8 else (False,)):
        bnd = D.trsm_update_bound(P, AP, X, R, U, alpha, t, nc, mfma)

        def worst(bug):
            got = m_xr(P, AP, X, R, U, alpha, t, nc, bug, mfma)
            return max(D.ratio(g, r, b) for g, r, b in zip(got, ref, bnd))

        bugs = ("last_row", "second_pass", "alpha_T", "inactive_col", "x_minus")
        report("trsm_update m=%d ts=%d t=%d %s" % (m, ts, t, "matrix cores" if mfma else "rows"), worst(None),
               {b: worst(b) for b in bugs if applies(b, m, t)})


@pytest.mark.parametrize("m", [7, 4099])
@pytest.mark.parametrize("ts", [2, 4, 8, 16])
def test_update_z_and_ztz(m, ts):
    """The plain update Z - [V0 | V1] beta and Z'^T Z' of the computed Z' (the by-product at 8 / 16 columns)."""
    rng = np.random.default_rng(m + ts)
    Z, V, beta = D.panel(rng, m, ts), D.panel(rng, m, 2 * ts), rng.standard_normal((2 * ts, ts))
    ref = D.update_z(Z, V, beta, ts)
    Za, cz = D.update_z_abs(Z, V, beta, ts)
    bnd = (cz + D.SPARE) * D.UNIT * Za

    def model(bug):
        b = beta.copy()
        if bug == "swap_g":
            b = np.vstack([beta[ts:], beta[:ts]])
        out = Z - V @ b
        if bug == "inactive_col":
            out[:, ts - 1] = Z[:, ts - 1]
        keep = rows_left_out(m, bug)
        out[keep] = Z[keep]
        return out

    bugs = [b for b in ("last_row", "second_pass", "swap_g", "inactive_col") if applies(b, m, ts)]
    report("update_z m=%d ts=%d" % (m, ts), D.ratio(model(None), ref, bnd), {b: D.ratio(model(b), ref, bnd) for b in bugs})
    gref, gbnd = D.gram(ref, ref), D.gram_bound(Za, Za, c_in=2 * cz + D.SPARE)
    zz = {b: model(b) for b in [None] + bugs}
    report("Z'^T Z' m=%d ts=%d" % (m, ts), D.ratio(zz[None].T @ zz[None], gref, gbnd),
           {b: D.ratio(zz[b].T @ zz[b], gref, gbnd) for b in bugs})


@pytest.mark.parametrize("nblk", [1, 63, 64, 65, 4174, 8193])
def test_sum_blocks(nblk):
    rng = np.random.default_rng(nblk)
    parts = rng.standard_normal((nblk, 32))
    ref, bnd = D.sum_blocks(parts), D.sum_blocks_bound(parts)
    report("sum_blocks nblk=%d" % nblk, D.ratio(m_sum(parts), ref, bnd),
           {b: D.ratio(m_sum(parts, b), ref, bnd) for b in ("drop_block", "double_block")})


@pytest.mark.parametrize("m", [1, 1000, 4099])
@pytest.mark.parametrize("na,nb", [(3, 3), (4, 4), (8, 5), (16, 16), (21, 12)])
def test_gram_and_colsums(m, na, nb):
    rng = np.random.default_rng(m + na + nb)
    A, B = rng.standard_normal((m, na)), rng.standard_normal((m, nb))
    chunk = 64
    blocks = np.stack([A[i:i + chunk].T @ B[i:i + chunk] for i in range(0, m, chunk)]).reshape(-(-m // chunk), -1)
    ref, bnd = D.gram(A, B).reshape(-1), D.gram_bound(A, B).reshape(-1)
    report("gram m=%d %dx%d" % (m, na, nb), D.ratio(m_sum(blocks), ref, bnd),
           {b: D.ratio(m_sum(blocks, b), ref, bnd) for b in ("drop_block", "double_block")})
    ref, bnd = D.colsums(B), D.colsums_bound(B)
    report("colsums m=%d n=%d" % (m, nb), D.ratio(m_sum(B), ref, bnd),
           {b: D.ratio(m_sum(B, b), ref, bnd) for b in ("drop_block", "double_block")})


@pytest.mark.parametrize("nblk", [1, 65, 8193])
@pytest.mark.parametrize("t", [1, 2, 3, 4, 7, 8, 15, 16])
def test_chol_alpha_backward(nblk, t):
    rng = np.random.default_rng(nblk + t)
    k = max(2 * t, 8)
    A, Bm = rng.standard_normal((nblk, k, t)), rng.standard_normal((nblk, k, t))
    Wp = np.einsum("bki,bkj->bij", A, A).reshape(nblk, -1)
    Gp = np.einsum("bki,bkj->bij", A, Bm).reshape(nblk, -1)          # G = P^T R, t x T
    W, G = m_sum(Wp).reshape(t, t), m_sum(Gp).reshape(t, t)
    Wr, Wb = D.sum_blocks(Wp).reshape(t, t), D.sum_blocks_bound(Wp).reshape(t, t)
    Gr, Gb = D.sum_blocks(Gp).reshape(t, t), D.sum_blocks_bound(Gp).reshape(t, t)
    mu, al = m_chol_alpha(W, G, t)
    good = max(D.chol_backward(mu, Wr, Wb, t), D.alpha_backward(mu, al, Gr, Gb, t))
    bad = {}
    mu2, al2 = m_chol_alpha(m_sum(Wp, "drop_block").reshape(t, t) if nblk > 1 else 0.5 * W, G, t)
    bad["drop_block"] = D.chol_backward(mu2, Wr, Wb, t)
    mu3, al3 = m_chol_alpha(W, m_sum(Gp, "double_block").reshape(t, t), t)
    bad["double_block"] = D.alpha_backward(mu3, al3, Gr, Gb, t)
    if t >= 2:
        bad["alpha_T"] = D.alpha_backward(mu, al.T, Gr, Gb, t)
    report("chol / alpha backward nblk=%d t=%d" % (nblk, t), good, bad)
