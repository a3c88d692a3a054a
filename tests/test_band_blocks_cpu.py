"""gen.band_blocks_csr: diagonal blocks with prescribed rows and bandwidth (the inputs of test_gpu_band_blocks.py).
Checked here, on the CPU: the exact band of every block, a block structure that matches `part`, symmetry in bits, the
factor the block was made from, and a Cholesky factorisation that succeeds on every block after symrac_scale."""
import numpy as np
import pytest
import scipy.sparse as sp

from prealps_amd import gen

BLOCKS = [(1, 0), (2, 1), (3, 5), (5, 4), (16, 15), (17, 5), (64, 33), (65, 64), (130, 112), (192, 0), (256, 80)]


def _dense_blocks(rp, ci, v, part, P):
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    out = []
    for q in range(P):
        idx = np.flatnonzero(part == q)
        out.append((idx, A[idx][:, idx].toarray(), A[idx][:, idx]))
    return A, out


def _band(D):
    i, j = np.nonzero(D)
    return int(np.abs(i - j).max()) if len(i) else 0


@pytest.mark.parametrize("grading", [0.0, 2.0, 3.0])
def test_rows_band_and_structure_are_the_prescribed_ones(grading):
    rp, ci, v, part, P = gen.band_blocks_csr(BLOCKS, seed=1, grading=grading)
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and v.dtype == np.float64 and part.dtype == np.int32
    assert P == len(BLOCKS) and len(part) == len(rp) - 1 == sum(b for b, _ in BLOCKS)
    assert np.array_equal(part, np.repeat(np.arange(P), [b for b, _ in BLOCKS]))      # contiguous, in the given order
    A, blocks = _dense_blocks(rp, ci, v, part, P)
    assert all(np.all(np.diff(ci[rp[i]:rp[i + 1]]) > 0) for i in range(len(rp) - 1))  # sorted, no duplicates
    assert sum(S.nnz for _, _, S in blocks) == A.nnz                                  # nothing outside the blocks
    for (b, w), (idx, D, S) in zip(BLOCKS, blocks):
        w = min(w, b - 1)
        assert D.shape == (b, b) and _band(D) == w
        i, j = np.indices((b, b))
        assert np.array_equal(D != 0, np.abs(i - j) <= w)                             # the band is full
        assert S.nnz == int((np.abs(i - j) <= w).sum())                               # and stored, nothing else


@pytest.mark.parametrize("kw", [dict(), dict(grading=3.0), dict(shuffle=True), dict(coupling=(2, 0.3)),
                                dict(grading=2.0, shuffle=True, coupling=(3, 0.1))])
def test_symmetric_in_bits(kw):
    rp, ci, v, part, P = gen.band_blocks_csr(BLOCKS, seed=2, **kw)
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    T = sp.csr_matrix(A.T)
    T.sort_indices()
    assert np.array_equal(T.indptr, A.indptr) and np.array_equal(T.indices, A.indices)
    assert np.array_equal(T.data.view(np.uint64), A.data.view(np.uint64))


@pytest.mark.parametrize("grading", [0.0, 3.0])
def test_blocks_are_the_product_of_the_documented_factor(grading):
    """The Cholesky factor of a block is L0 up to the signs of its columns (the diagonal of L0 is positive: it is L0):
    diagonal in [1, 2] or [10^(-g/4), 10^(g/4)], sub-diagonal magnitudes in [0.25, 1] / sqrt(w + 1), both signs."""
    rp, ci, v, part, P = gen.band_blocks_csr(BLOCKS, seed=3, grading=grading)
    _, blocks = _dense_blocks(rp, ci, v, part, P)
    neg = pos = 0
    for (b, w), (idx, D, S) in zip(BLOCKS, blocks):
        w = min(w, b - 1)
        L = np.linalg.cholesky(D)
        d = np.diag(L)
        lo, hi = (1.0, 2.0) if grading == 0 else (10.0 ** (-grading / 4), 10.0 ** (grading / 4))
        assert np.all(d >= lo * (1 - 1e-9)) and np.all(d <= hi * (1 + 1e-9))
        i, j = np.indices((b, b))
        sub = L[(i > j) & (i - j <= w)]
        s = np.sqrt(w + 1.0)
        tol = 1e-9 * hi / lo
        assert np.all(np.abs(sub) * s >= 0.25 - tol) and np.all(np.abs(sub) * s <= 1.0 + tol)
        assert np.all(L[(i - j) > w] == 0)
        neg += int((sub < 0).sum())
        pos += int((sub > 0).sum())
    assert neg > 0.4 * (neg + pos) and pos > 0.4 * (neg + pos)


def test_bandwidth_above_the_rows_is_clipped_and_the_seed_decides():
    a = gen.band_blocks_csr([(4, 9), (1, 3)], seed=5)
    b = gen.band_blocks_csr([(4, 3), (1, 0)], seed=5)
    c = gen.band_blocks_csr([(4, 3), (1, 0)], seed=6)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] == 2
    assert len(a[2]) == 16 + 1 and not np.array_equal(b[2], c[2])
    with pytest.raises(ValueError):
        gen.band_blocks_csr([], seed=0)
    with pytest.raises(ValueError):
        gen.band_blocks_csr([(0, 0)], seed=0)


def test_shuffle_keeps_the_rows_and_the_spectrum():
    """A symmetric permutation inside every block: the same rows per block, the same number of entries, the same
    eigenvalues as a block L0 L0^T of that band -- and a band that is no longer the prescribed one."""
    rp, ci, v, part, P = gen.band_blocks_csr(BLOCKS, seed=7, shuffle=True)
    _, blocks = _dense_blocks(rp, ci, v, part, P)
    wider = 0
    for (b, w), (idx, D, S) in zip(BLOCKS, blocks):
        w = min(w, b - 1)
        i, j = np.indices((b, b))
        assert D.shape == (b, b) and S.nnz == int((np.abs(i - j) <= w).sum())
        assert _band(D) >= w
        wider += _band(D) > w
        assert np.linalg.eigvalsh(D).min() > 0
    assert wider == sum(1 for b, w in BLOCKS if 0 < w < b - 1)      # (a diagonal or a full block has no other band)


def test_coupling_leaves_the_blocks_band_and_the_sum_positive_definite():
    plain = gen.band_blocks_csr(BLOCKS, seed=8, grading=2.0)
    rp, ci, v, part, P = gen.band_blocks_csr(BLOCKS, seed=8, grading=2.0, coupling=(2, 0.4))
    A0, b0 = _dense_blocks(*plain)
    A, b1 = _dense_blocks(rp, ci, v, part, P)
    off = A.nnz - sum(S.nnz for _, _, S in b1)
    assert off > 0 and off % 2 == 0
    rows = np.repeat(np.arange(A.shape[0]), np.diff(rp))
    out = part[rows] != part[ci]
    assert np.all(np.abs(v[out]) >= 0.2 - 1e-15) and np.all(np.abs(v[out]) <= 0.4)
    absrow = np.zeros(A.shape[0])
    np.add.at(absrow, rows[out], np.abs(v[out]))
    for (idx, D0, _), (_, D1, _) in zip(b0, b1):
        E = D1 - D0
        assert np.array_equal(E, np.diag(np.diag(E)))                       # only the diagonal of a block moved
        np.testing.assert_allclose(np.diag(E), absrow[idx], rtol=1e-12, atol=1e-15)   # by the sum of |c| of the row
    assert np.linalg.eigvalsh(A.toarray()).min() > 0


@pytest.mark.parametrize("kw", [dict(), dict(grading=2.0), dict(grading=3.0), dict(grading=3.0, shuffle=True),
                                dict(grading=3.0, coupling=(2, 0.4))])
def test_every_block_factors_after_scaling(kw):
    """What the GPU tests build: symrac_scale, permute_by_part (the identity here), Cholesky of every diagonal block;
    and the oracle's own block factorisation accepts the matrix."""
    from oracle import oracle as O
    rp, ci, v, part, P = gen.band_blocks_csr(BLOCKS, seed=9, **kw)
    N = len(rp) - 1
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(sp.csr_matrix((v, ci, rp), shape=(N, N))), part, P)
    assert np.array_equal(perm, np.arange(N))
    assert np.array_equal(np.diff(rowpos), [b for b, _ in BLOCKS])
    for q in range(P):
        D = B[rowpos[q]:rowpos[q + 1], rowpos[q]:rowpos[q + 1]].toarray()
        L = np.linalg.cholesky(D)
        assert np.isfinite(L).all() and np.diag(L).min() > 0
        assert np.abs(D).max() <= 1.0 + 1e-15                                # scaled: no entry above 1
    X = np.random.default_rng(0).standard_normal((N, 2))
    Z = O.BlockJacobi(B, rowpos).apply(X)
    assert np.isfinite(Z).all()


@pytest.mark.parametrize("name,grading,delta", [("depth64", 0.0, 1e-10), ("mixed", 3.0, 1e-6)])
def test_the_backward_error_criterion_tells_a_wrong_factor_entry(name, grading, delta):
    """The criterion of test_gpu_band_blocks.py on solves made here: the oracle's solve and a numpy Cholesky solve stay
    under (3 w + 16) u on well-conditioned and on graded blocks (condition 1e7); one factor entry per block that is
    dropped, or wrong by 1e-10 relative (1e-6 on graded blocks, where the entry's share of its row of |L| |L|^T can
    be small), puts omega above the limit in every block; a factor rounded to fp32 exceeds the fp64 limit
    and stays under the fp32 one."""
    import scipy.linalg as sl
    import test_gpu_band_blocks as T
    c = T._case(name, grading, False)
    X, Zo, om_o = T._reference(name, grading, False, 4)
    limit = np.array([(3 * w + 16) * T.U for b, w in c.blocks])
    assert np.all(om_o <= limit)

    def omega(change):
        Z = np.empty_like(Zo)
        for q in range(c.P):
            r0, r1 = c.rowpos[q], c.rowpos[q + 1]
            L = np.linalg.cholesky(np.asarray(c.A[q], dtype=np.float64))
            L = change(L, r1 - r0, c.blocks[q][1])
            Z[r0:r1] = sl.solve_triangular(L.T, sl.solve_triangular(L, X[r0:r1], lower=True), lower=False)
        return T._omega(c, X, Z)

    def entry(factor):
        def change(L, b, w):
            if b > 2 and w > 0:
                L[b // 2, b // 2 - 1] *= factor
            return L
        return change

    def single(L, b, w):
        d = np.diag(L).copy()
        return (L / d).astype(np.float32).astype(np.float64) * d

    banded = np.array([b > 2 and w > 0 for b, w in c.blocks])
    assert np.all(omega(lambda L, b, w: L) <= limit)
    assert np.all(omega(entry(0.0))[banded] > 1e6 * limit[banded])
    assert np.all(omega(entry(1 + delta))[banded] > limit[banded])
    om32 = omega(single)
    assert np.all(om32[banded] > limit[banded]) and np.all(om32 <= limit + 2.0 ** -23 * 1.01)
