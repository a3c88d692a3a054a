"""References and error bounds for the solution history (not collected: no test_ prefix).

u = 2^-53, gamma_n = n u / (1 - n u).  Every bound is evaluated in longdouble from the data of the test itself.

  dots     |fl(x^T w) - x^T w| <= gamma_N sum_r |x_r||w_r| for any order of summation (fma or not); the mapped form
           divides w by d first, one more rounding per term, and reads a product that was itself rounded on its way
           out of the scaled space: gamma_(N+2).
  combine  |fl(Xh c) - Xh c|_r <= gamma_K sum_i |X_ri||c_i|.
  Galerkin rho_i = x_i^T (b - A x0) / ||x_i||_A on the columns the projection kept.  Exactly, G c = g gives rho = 0.
           Computed: with s_i = 1 / ||x_i||_A, Gs = S G^ S, gs = S g^, the Cholesky solve leaves (Higham, Accuracy and
           Stability, Thm 10.4) |Gs cs - gs|_i <= gamma_(3K+1) (|R^T||R| |cs|)_i <= gamma_(3K+1) (1 + eps) ||cs||_1,
           because the columns of R have norm sqrt(Gs_jj) ~ 1.  Splitting
             s_i (g_i - (G c)_i) = s_i (g_i - g^_i) + (gs - Gs cs)_i + (S (G^ - G) S cs)_i
           gives |rho_i| <= (gamma_(3K+1) + eta_G) ||cs||_1 + eta_g,i with
             eta_G   = max_ij s_i s_j |G^_ij - G_ij|, |G^_ij - G_ij| <= (gamma_(N+2) + gamma_(nmax+3)) |x_i|^T |A| |x_j|
                       (the dot, and the product w = A x: two roundings of the scaling of an entry, one of x / d, nmax
                       terms of the row sum),
             eta_g,i = s_i gamma_N |x_i|^T |b|.
           Two more constants are needed, both named here: SCALE_U = 8 u on every entry of Gs and 4 u on gs and c for the
           roundings of s_i = 1 / sqrt(G^_ii) and of the two multiplications that scale an entry (entries of Gs are at
           most 1 in size); and eta_c,i = s_i gamma_K |x_i|^T |A| |Xh||c| for the rounding of the combine x0 = Xh c, which
           the Galerkin residual sees through A.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
SCALE_U = 8 * U


def gamma(n):
    return LD(n) * LD(U) / (LD(1) - LD(n) * LD(U))


def dots_exact(X, W):
    return X.astype(LD).T @ W.astype(LD)


def dots_bound(X, W, n_terms):
    return gamma(n_terms) * (np.abs(X).astype(LD).T @ np.abs(W).astype(LD))


def combine_exact(X, c):
    return X.astype(LD) @ c.astype(LD)


def combine_bound(X, c):
    return gamma(X.shape[1]) * (np.abs(X).astype(LD) @ np.abs(c).astype(LD))


# ---- a float64 restatement of the history: ring, Gram matrix, scaled pivoted Cholesky -------------------------------
def pivoted_cholesky_solve(Gs, gs, rtol):
    """Diagonally pivoted Cholesky of the unit-diagonal Gs, stopping when the largest remaining pivot is <= rtol;
    returns (kept columns in pivot order, cs with zeros at the dropped ones)."""
    K = Gs.shape[0]
    d = np.diag(Gs).copy()
    R = np.zeros((0, K))
    piv = []
    while len(piv) < K:
        rest = [j for j in range(K) if j not in piv]
        p = max(rest, key=lambda j: (d[j], -j))
        if not d[p] > rtol:
            break
        row = np.zeros(K)
        row[p] = np.sqrt(d[p])
        for j in rest:
            if j != p:
                row[j] = (Gs[p, j] - R[:, p] @ R[:, j]) / row[p]
                d[j] -= row[j] ** 2
        R = np.vstack([R, row])
        piv.append(p)
    cs = np.zeros_like(gs)
    if piv:
        Rk = R[:, piv]
        cs[piv] = np.linalg.solve(Rk, np.linalg.solve(Rk.T, gs[piv]))
    return piv, cs


class RefHistory:
    """Columns in ring (logical) order, oldest first; G in the same order.  matvec(X) = A X in the caller's units."""

    def __init__(self, capacity, matvec, dot=None):
        self.cap, self.matvec = capacity, matvec
        self.dot = dot if dot is not None else (lambda X, W: X.T @ W)
        self.X = None
        self.G = np.zeros((0, 0))

    @property
    def count(self):
        return 0 if self.X is None else self.X.shape[1]

    def append(self, Xn):
        Xn = np.asarray(Xn, dtype=np.float64).reshape(len(Xn), -1)[:, -self.cap:]
        W = self.matvec(Xn)
        old = self.X if self.X is not None else np.zeros((Xn.shape[0], 0))
        K, q = old.shape[1], Xn.shape[1]
        G = np.zeros((K + q, K + q))
        G[:K, :K] = self.G
        G[:K, K:] = self.dot(old, W)
        nn = self.dot(Xn, W)
        G[K:, K:] = np.triu(nn)
        G = np.triu(G) + np.triu(G, 1).T
        X = np.hstack([old, Xn])
        drop = max(0, X.shape[1] - self.cap)
        self.X, self.G = X[:, drop:], G[drop:, drop:]

    def refresh(self):
        if self.count:
            G = np.triu(self.dot(self.X, self.matvec(self.X)))
            self.G = G + np.triu(G, 1).T

    def project(self, B, rtol=1e-12):
        """(x0, rank, captured, kept, c, cs): kept = the logical columns the Cholesky kept."""
        B = np.asarray(B, dtype=np.float64).reshape(len(B), -1)
        if not self.count:
            return np.zeros_like(B), 0, np.zeros(B.shape[1]), [], np.zeros((0, B.shape[1])), np.zeros((0, B.shape[1]))
        g = self.dot(self.X, B)
        dg = np.diag(self.G)
        s = np.where(dg > 0, 1.0 / np.sqrt(np.where(dg > 0, dg, 1.0)), 0.0)
        Gs = (self.G * s[:, None]) * s[None, :]
        np.fill_diagonal(Gs, (s > 0).astype(float))
        kept, cs = pivoted_cholesky_solve(Gs, g * s[:, None], rtol)
        c = cs * s[:, None]
        return self.X @ c, len(kept), (c * g).sum(axis=0), kept, c, cs


# ---- the Galerkin defect and its bound ------------------------------------------------------------------------------
def galerkin(A, absA, n_max, X, kept, b, x0, c, with_combine=True):
    """(rho, bound) for one right-hand side: X the history columns (logical order), kept the columns the projection
    kept, c its coefficients (zeros at the dropped columns), all float64; A, absA scipy matrices in the caller's units."""
    K, N = X.shape[1], X.shape[0]
    AX = np.asarray(A @ X)
    absAX = np.asarray(absA @ np.abs(X)).astype(LD)
    Gd = np.einsum("ri,ri->i", X.astype(LD), AX.astype(LD))
    s = np.where(Gd > 0, LD(1) / np.sqrt(np.where(Gd > 0, Gd, LD(1))), LD(0))
    r = b.astype(LD) - np.asarray(A @ x0).astype(LD)
    # (b - A x0 in float64 products carries gamma_nmax |A||x0|: counted with the bound, not with the defect)
    r_err = gamma(n_max + 1) * (np.abs(b).astype(LD) + np.asarray(absA @ np.abs(x0)).astype(LD))
    rho = (X.astype(LD).T @ r) * s
    cs = np.where(s > 0, np.abs(c).astype(LD) / np.where(s > 0, s, LD(1)), LD(0))
    absX = np.abs(X).astype(LD)
    eta_G = ((gamma(N + 2) + gamma(n_max + 3)) * (absX.T @ absAX) * s[:, None] * s[None, :]).max() + LD(SCALE_U)
    eta_g = gamma(N) * (absX.T @ np.abs(b).astype(LD)) * s + LD(4 * U) * np.abs((X.astype(LD).T @ b.astype(LD)) * s)
    eta_c = gamma(K) * (absAX.T @ (absX @ np.abs(c).astype(LD))) * s if with_combine else LD(0)
    meas = (absX.T @ r_err) * s
    bound = (LD(1.01) * gamma(3 * K + 1) + eta_G) * cs.sum() * LD(1 + 4 * U) + eta_g + eta_c + meas
    return rho[kept], bound[kept]


def energy_norm(A, v):
    return float(np.sqrt(max(float(v.astype(LD) @ np.asarray(A @ v).astype(LD)), 0.0)))


# ---- the NumPy restatement of Orthodir with a start (tests/test_gpu_warm_start.py), on one matrix ---------------------
def split(V, rowpos, s):
    N, k = V.shape
    out = np.zeros((N, k * s))
    for p in range(len(rowpos) - 1):
        for j in range(k):
            out[rowpos[p]:rowpos[p + 1], j * s + p % s] = V[rowpos[p]:rowpos[p + 1], j]
    return out


def restate(A, rowpos, inv, B, s, X0=None, tol=1e-5, max_iter=500):
    """Orthodir on R0 = split(B) or, from a guess, X = split(X0) and R0 = split(B - group sums of A X).  Returns the
    per-system history (iterations x k, absolute), the k solutions, ||b_j|| and the start residual norms."""
    N, k = B.shape
    t, nparts = k * s, len(rowpos) - 1

    def precond(X):
        Y = np.empty_like(X)
        for p in range(nparts):
            Y[rowpos[p]:rowpos[p + 1]] = inv[p] @ X[rowpos[p]:rowpos[p + 1]]
        return Y

    if X0 is None:
        X, R = np.zeros((N, t)), split(B, rowpos, s)
    else:
        X = split(X0, rowpos, s)
        R = split(B - (A @ X).reshape(N, k, s).sum(axis=2), rowpos, s)
    nb = np.linalg.norm(B, axis=0)
    g0 = np.sqrt((R ** 2).reshape(N, k, s).sum(axis=(0, 2)))
    hist = []
    if not (g0 > tol * nb).any():
        return np.zeros((0, k)), X.reshape(N, k, s).sum(axis=2), nb, g0
    Pm, Pp, APp = precond(R), np.zeros((N, t)), np.zeros((N, t))
    for _ in range(max_iter):
        AP = A @ Pm
        Uf = np.linalg.cholesky(Pm.T @ AP).T
        Pm, AP = np.linalg.solve(Uf.T, Pm.T).T, np.linalg.solve(Uf.T, AP.T).T
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
    return np.array(hist), X.reshape(N, k, s).sum(axis=2), nb, g0


# ---- the heat sequence: implicit Euler on the 10^3 Poisson grid ------------------------------------------------------
HEAT_N, HEAT_DT, HEAT_PARTS, HEAT_T, HEAT_TOL, HEAT_STEPS = 10, 5.0, 8, 4, 1e-5, 16


def heat_matrix():
    """A = I + 5 K (K: the 7-point Poisson matrix of the 10^3 grid), its CSR arrays and the 8 contiguous parts."""
    import scipy.sparse as sp
    from prealps_amd import gen
    rp, ci, v = gen.poisson3d_csr(HEAT_N)
    N = len(rp) - 1
    A = (sp.identity(N, format="csr") + HEAT_DT * sp.csr_matrix((v, ci, rp), shape=(N, N))).tocsr()
    A.sort_indices()
    rowpos = np.array([(N * p) // HEAT_PARTS for p in range(HEAT_PARTS + 1)], dtype=np.int64)
    return A, rowpos


def heat_source(tm):
    """A travelling sine plus a moving Gaussian on the unit cube, at time tm."""
    n = HEAT_N
    g = (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    sine = np.sin(2 * np.pi * (x - 0.3 * tm)) * np.sin(np.pi * y) * np.sin(np.pi * z)
    cx, cy = 0.5 + 0.3 * np.cos(0.25 * tm), 0.5 + 0.3 * np.sin(0.25 * tm)
    gauss = np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - 0.5) ** 2) / 0.02)
    return (sine + gauss).ravel()


def heat_rhs(u_prev, step):
    return u_prev + HEAT_DT * heat_source(0.2 * step)


def heat_reference():
    """The 16 steps by the restatement, cold and with a history of 8: per step the iterations of both, the start x0 of
    the history run (None where the history is empty) and its solutions.  The two runs advance on their own solutions."""
    A, rowpos = heat_matrix()
    inv = [np.linalg.inv(A[r0:r1, r0:r1].toarray()) for r0, r1 in zip(rowpos[:-1], rowpos[1:])]
    N = A.shape[0]
    out = dict(cold=[], hist=[], x0=[], b=[], x=[], g0=[], nb=[])
    uc, uh = np.zeros(N), np.zeros(N)
    H = RefHistory(8, lambda X: np.asarray(A @ X))
    for n in range(1, HEAT_STEPS + 1):
        bc = heat_rhs(uc, n)
        hc, xc, _, _ = restate(A, rowpos, inv, bc[:, None], HEAT_T, tol=HEAT_TOL)
        uc = xc[:, 0]
        bh = heat_rhs(uh, n)
        x0, rank, _, _, _, _ = H.project(bh)
        hh, xh, nb, g0 = restate(A, rowpos, inv, bh[:, None], HEAT_T, X0=x0 if rank else None, tol=HEAT_TOL)
        uh = xh[:, 0]
        if len(hh):
            H.append(uh)
        out["cold"].append(len(hc)); out["hist"].append(len(hh)); out["x0"].append(x0[:, 0] if rank else None)
        out["b"].append(bh); out["x"].append(uh.copy()); out["g0"].append(float(g0[0])); out["nb"].append(float(nb[0]))
    return out
