"""References and error bounds of the dense panel kernels (dense_update.hip, dense_gram.hip), for
test_dense_ref_cpu.py (no GPU: the bounds hold for a float64 restatement and catch seeded mistakes) and for
test_gpu_row_pass.py, test_gpu_gram_finish.py and test_gpu_dense_kernels.py (the kernels themselves).

Everything here works in np.longdouble from float64 inputs.  A panel is a (rows, ts) array, row-interleaved as on the
device, of which the first t columns are active; a small block (U, alpha, beta, W) is a plain 2-D array, (i, j) = row,
column -- the callers lay it out column-major for the device.

The bound of an entry is  c * 2^-53 * (the same expression on absolute values),  where the inverse of a triangular
factor is replaced by the inverse of its comparison matrix (diagonal |u_ii|, off-diagonal -|u_ij|: a nonnegative
matrix that dominates |U^-1| and every intermediate of a substitution).  c counts the roundings on the longest
dependency chain to the entry; it composes as
    sum:       c(x + y)  = max(c_x, c_y) + 1        (a sum of n terms, in any order: max c + n - 1)
    product:   c(x * y)  = c_x + c_y + 1            (and the same for a quotient)
to first order in 2^-53, by induction over the expression.  A multiply-add is counted as a product and a sum, so a
count holds with and without fused multiply-add.  SPARE = 2 units are added to every count for the second-order terms,
as in test_gpu_spmm_blocks.py.  Every count below is taken from the kernels' loops; none from a run.

Not a test module: nothing here is collected."""
import numpy as np

LD = np.longdouble
UNIT = 2.0 ** -53
SPARE = 2
WG = 256                  # threads of a workgroup (kernels_common.h)
UPDATE_CAP = 512          # workgroups of the row pass at the most (GRAM_MAX_BLOCKS)


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------------------------------- small blocks ----
def inv_upper(U, dtype=LD):
    """U^-1 of an upper-triangular U by back substitution on the unit vectors."""
    U = np.asarray(U, dtype=dtype)
    t = U.shape[0]
    inv = np.zeros((t, t), dtype=dtype)
    for c in range(t):
        for i in range(c, -1, -1):
            s = dtype(1.0) if i == c else dtype(0.0)
            for k in range(i + 1, c + 1):
                s = s - U[i, k] * inv[k, c]
            inv[i, c] = s / U[i, i]
    return inv


def comparison_inverse(U):
    """Inverse of the comparison matrix of U: >= |U^-1| entry by entry, and nonnegative."""
    A = np.abs(ld(U))
    M = -np.triu(A, 1) + np.diag(np.diag(A))
    return inv_upper(M)


def cond_upper(U):
    return float(np.linalg.cond(np.asarray(U, dtype=np.float64)))


def update_grid(m):
    """Workgroups of the row pass (update_grid of dense_device.h: two rows per lane, capped)."""
    return min(UPDATE_CAP, max(1, -(-m // (2 * WG))))


def passes(m, nblk=None):
    """Rows a lane of the row pass takes at the most (its grid-stride loop)."""
    nblk = update_grid(m) if nblk is None else nblk
    return max(1, -(-m // (nblk * WG)))


def factor(rng, t):
    """An upper-triangular factor as the tests use them: triu(randn) + 4 I, condition number below 1e3 (asserted)."""
    U = np.triu(rng.standard_normal((t, t))) + 4.0 * np.eye(t)
    assert cond_upper(U) < 1e3
    return U


def panel(rng, m, ts):
    return rng.standard_normal((m, ts))


# ------------------------------------------------------------------------------------------------ counts ----
def c_subst(t):
    """p <- p U^-1 along a row (trsm_update_row): p_0 = p_0 * (1 / u_00) is 2 roundings; p_j takes off j terms
    p_k u_kj -- the last one carries c(p_{j-1}) + 1 and its subtraction 1 more -- then the product with the rounded
    reciprocal, 2: c(p_j) = c(p_{j-1}) + 4, so 4 t - 2 at column t - 1."""
    return 4 * t - 2


def c_xr(t):
    """x_c += sum_k p_k alpha_kc (and r): product with alpha: c_subst + 1; sum of t terms and x itself: + t."""
    return c_subst(t) + 1 + t + SPARE


def c_inv(t):
    """A column of U^-1 by back substitution (lazy_coeffs_wg, lazy_coeffs16, k_trsm_update_mfma): the diagonal entry
    1 / u_cc is 1 rounding; the entry d places above it takes off d terms, the first of which carries the entry
    below (+ 1 product, + 1 subtraction), each further one 1 subtraction, then the division:
    b_d = b_{d-1} + d + 2, b_0 = 1, so 1 + d (d + 1) / 2 + 2 d at d = t - 1."""
    d = t - 1
    return 1 + d * (d + 1) // 2 + 2 * d


def c_lazy_z(t, a_hi):
    """Z' = Z C0 - V0 C1 - V1 C2 (lazy_coeffs_*, update_z_lazy_row, the matrix-core loops):
    T = G Ui: product c_inv + 1, t terms: c_inv + t;   beta = Ui^T T: c_inv + (c_inv + t) + 1, t terms: 2 c_inv + 2 t;
    C1 = Ui beta: 3 c_inv + 3 t (C2 alike, C0 = Ui: c_inv);
    a row: n = 3 t terms (2 t without V1), the largest a product with C1: 3 c_inv + 3 t + 1 + n - 1."""
    n = (3 if a_hi else 2) * t
    return 3 * c_inv(t) + 3 * t + n + SPARE


def c_colsum(t, npass):
    """Column sums of R'^2 per workgroup (block_sum_cols): r^2 of a computed r: 2 (c_xr - SPARE) + 1; a lane adds
    npass of them, the wavefront folds in 6 steps, the four wavefronts in 3."""
    return 2 * (c_xr(t) - SPARE) + 1 + npass + 6 + 3 + SPARE


def c_trace(t, npass, nblk, nc):
    """k_trace_finish / trace_finish_wg on those sums: a thread adds ceil(nblk / 256) nc of them, the tree has 8 levels."""
    return c_colsum(t, npass) + (-(-nblk // WG)) * nc + 8


def c_trsm_mfma(t):
    """k_trsm_update_mfma: B = Ui alpha: c_inv + 1, t terms: c_inv + t; X += P B: + 1, t terms and x: + t.
    (P Ui: c_inv + t.)"""
    return c_inv(t) + 2 * t + 1 + SPARE


def c_chol(t):
    """mu^T mu = W backward (potrf_upper_wg, both of its paths are dpotf2's operations): entry (i, j) takes off at
    most t - 1 products and is divided once or goes through one square root: t + 1 (Higham, Accuracy and Stability
    of Numerical Algorithms, Theorem 10.3)."""
    return t + 1 + SPARE


def c_alpha(t):
    """mu^T alpha = G backward (potrf_alpha_wg's substitution: t - 1 products taken off, one division: t, ibid.
    Theorem 8.5, any order)."""
    return t + SPARE


# ----------------------------------------------------------------------------------------------- row pass ----
def _coeffs(U, Uprev, beta, t, a_hi, absolute):
    f = np.abs if absolute else (lambda a: a)
    inv = comparison_inverse if absolute else inv_upper
    Ui = inv(ld(U)[:t, :t])
    G1 = f(ld(beta)[:t, :t])
    C1 = Ui @ (Ui.T @ G1 @ Ui)
    C2 = None
    if a_hi:
        Up = inv(ld(Uprev)[:t, :t])
        G2 = f(ld(beta)[t:2 * t, :t])
        C2 = Up @ (Up.T @ G2 @ Ui)
    return Ui, C1, C2


def _lazy_z(Z, V0, V1, U, Uprev, beta, t, absolute):
    f = np.abs if absolute else (lambda a: a)
    sg = 1 if absolute else -1
    Ui, C1, C2 = _coeffs(U, Uprev, beta, t, 0 if V1 is None else t, absolute)
    Zo = f(ld(Z)).copy()
    act = Zo[:, :t] @ Ui + sg * (f(ld(V0)[:, :t]) @ C1)
    if V1 is not None:
        act = act + sg * (f(ld(V1)[:, :t]) @ C2)
    Zo[:, :t] = act
    return Zo


def lazy_update_z(Z, V0, V1, U, Uprev, beta, t):
    """Z' = Z Ui - V0 Ui (Ui^T G1 Ui) - V1 Up (Up^T G2 Ui), beta = [G1 ; G2]; without V1 the third term is absent."""
    return _lazy_z(Z, V0, V1, U, Uprev, beta, t, False)


def lazy_update_z_bound(Z, V0, V1, U, Uprev, beta, t):
    b = c_lazy_z(t, 0 if V1 is None else t) * UNIT * _lazy_z(Z, V0, V1, U, Uprev, beta, t, True)
    b[:, t:] = 0
    return b


def _xr(P, AP, X, R, U, alpha, t, nc, absolute):
    f = np.abs if absolute else (lambda a: a)
    sg = 1 if absolute else -1
    Ui = (comparison_inverse if absolute else inv_upper)(ld(U)[:t, :t])
    a = f(ld(alpha)[:t, :nc])
    Pn, APn = f(ld(P)).copy(), f(ld(AP)).copy()
    Pn[:, :t] = Pn[:, :t] @ Ui
    APn[:, :t] = APn[:, :t] @ Ui
    Xo, Ro = f(ld(X)).copy(), f(ld(R)).copy()
    Xo[:, :nc] = Xo[:, :nc] + Pn[:, :t] @ a
    Ro[:, :nc] = Ro[:, :nc] + sg * (APn[:, :t] @ a)
    S = np.zeros(Ro.shape[1], dtype=LD)
    S[:nc] = (Ro[:, :nc] ** 2).sum(axis=0)
    return Pn, APn, Xo, Ro, S


def row_pass(P, AP, Pprev, X, R, Z, U, alpha, beta, Uprev, t):
    """X' = X + (P Ui) alpha, R' = R - (AP Ui) alpha, Z' as lazy_update_z with V0 = P, V1 = Pprev, and the column sums
    of R'^2; columns >= t unchanged, their sums 0."""
    _, _, Xo, Ro, S = _xr(P, AP, X, R, U, alpha, t, t, False)
    return Xo, Ro, lazy_update_z(Z, P, Pprev, U, Uprev, beta, t), S


def row_pass_bound(P, AP, Pprev, X, R, Z, U, alpha, beta, Uprev, t, npass=None):
    """Bounds of row_pass's four results; npass = rows per lane (passes(m) of the kernel's grid)."""
    npass = passes(P.shape[0]) if npass is None else npass
    _, _, Xa, Ra, Sa = _xr(P, AP, X, R, U, alpha, t, t, True)
    bX, bR = c_xr(t) * UNIT * Xa, c_xr(t) * UNIT * Ra
    bX[:, t:] = 0
    bR[:, t:] = 0
    return bX, bR, lazy_update_z_bound(Z, P, Pprev, U, Uprev, beta, t), c_colsum(t, npass) * UNIT * Sa


def trace_bound(P, AP, X, R, U, alpha, t, nblk, nc, npass=None):
    """Bound of res2[0] = the sum of the first nc column sums, as k_trace_finish adds them."""
    npass = passes(P.shape[0], nblk) if npass is None else npass
    Sa = _xr(P, AP, X, R, U, alpha, t, t, True)[4]
    return c_trace(t, npass, nblk, nc) * UNIT * Sa[:nc].sum()


def owed_x(X, Pprev, Uprev, akeep, t):
    """X + (Pprev Up) akeep: the update a skipping pass owes."""
    return _xr(Pprev, Pprev, X, X, Uprev, akeep, t, t, False)[2]


def owed_x_bound(X, Pprev, Uprev, akeep, t):
    b = c_xr(t) * UNIT * _xr(Pprev, Pprev, X, X, Uprev, akeep, t, t, True)[2]
    b[:, t:] = 0
    return b


def trsm_update(P, AP, X, R, U, alpha, t, nc):
    """P Ui, AP Ui, X + (P Ui) alpha, R - (AP Ui) alpha, column sums of the new R^2 (t columns of P, nc of X)."""
    return _xr(P, AP, X, R, U, alpha, t, nc, False)


def trsm_update_bound(P, AP, X, R, U, alpha, t, nc, matrix_cores):
    """Bounds of P, AP, X, R.  matrix_cores: the 8 / 16-column kernel, which forms Ui and Ui alpha first."""
    Pa, APa, Xa, Ra, _ = _xr(P, AP, X, R, U, alpha, t, nc, True)
    cp = (c_inv(t) + t if matrix_cores else c_subst(t)) + SPARE
    cx = c_trsm_mfma(t) if matrix_cores else c_xr(t)
    out = [cp * UNIT * Pa, cp * UNIT * APa, cx * UNIT * Xa, cx * UNIT * Ra]
    out[0][:, t:] = 0
    out[1][:, t:] = 0
    out[2][:, nc:] = 0
    out[3][:, nc:] = 0
    return out


def update_z(Z, V, beta, nc):
    """Z(:, :nc) - V beta, V = the active columns of [V0 | V1] side by side (the plain update)."""
    Zo = ld(Z).copy()
    Zo[:, :nc] = Zo[:, :nc] - ld(V) @ ld(beta)[:, :nc]
    return Zo


def update_z_abs(Z, V, beta, nc):
    """update_z on absolute values, and its count: na products taken off z: na + 1."""
    Za = np.abs(ld(Z))
    Za[:, :nc] = Za[:, :nc] + np.abs(ld(V)) @ np.abs(ld(beta))[:, :nc]
    return Za, V.shape[1] + 1


# --------------------------------------------------------------------------------------------------- sums ----
def sum_blocks(parts):
    """Sum of a (nblk, n) stack of partial blocks."""
    return ld(parts).sum(axis=0)


def sum_blocks_bound(parts):
    """nblk * 2^-53 * sum |block|: nblk - 1 additions in whatever order."""
    p = ld(parts)
    return p.shape[0] * UNIT * np.abs(p).sum(axis=0)


def gram(A, B):
    return ld(A).T @ ld(B)


def gram_bound(A, B, c_in=0):
    """m * 2^-53 * |A|^T |B|: a product and m - 1 additions in whatever order; c_in: roundings already in A and B
    (A, B then their absolute evaluations)."""
    return (A.shape[0] + c_in) * UNIT * (np.abs(ld(A)).T @ np.abs(ld(B)))


def colsums(R):
    return ld(R).sum(axis=0)


def colsums_bound(R):
    return R.shape[0] * UNIT * np.abs(ld(R)).sum(axis=0)


# ----------------------------------------------------------------------------- Cholesky and alpha: backward ----
def chol_backward(mu, W, W_bound, t):
    """Worst ratio of |mu^T mu - W| to c_chol u |mu|^T |mu| + W_bound on the leading t x t; mu is taken as upper
    triangular (what lies below its diagonal is the caller's to judge)."""
    m = np.triu(ld(mu)[:t, :t])
    lim = c_chol(t) * UNIT * (np.abs(m).T @ np.abs(m)) + ld(W_bound)[:t, :t]
    return ratio(m.T @ m, ld(W)[:t, :t], lim)


def alpha_backward(mu, alpha, G, G_bound, t):
    """Worst ratio of |mu^T alpha - G| to c_alpha u |mu|^T |alpha| + G_bound; alpha and G are t x T."""
    m = np.triu(ld(mu)[:t, :t])
    lim = c_alpha(t) * UNIT * (np.abs(m).T @ np.abs(ld(alpha))) + ld(G_bound)
    return ratio(m.T @ ld(alpha), ld(G), lim)


def ratio(got, ref, bound):
    """max |got - ref| / bound; 0 where both are 0, inf where only the bound is (or where got is not finite)."""
    got, ref, bound = ld(got), ld(ref), ld(bound)
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q)) if q.size else 0.0
