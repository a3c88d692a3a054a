"""Single-precision storage of the sparse (nested-dissection) block factor: PREALPS_BJ_ND_PRECISION=single,
preAlps_hip_set_nd_precision(32), EcgProblem.create_block_jacobi(nd_precision="single").  The factor is computed in
fp64, both panel copies are rounded to fp32 from the same values, and the apply widens every coefficient and keeps all
of its arithmetic in fp64.  Band blocks stay fp64.  Unset, everything computes the same bits as before."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SW = "PREALPS_BJ_ND_PRECISION"


def _random_blocks():
    """The blocks of test_large_blocks_that_are_no_grids: a random pattern, nearest-neighbour links of random points,
    two disconnected halves, and a few couplings between the blocks."""
    from scipy.spatial import cKDTree
    nb, P = 2600, 4
    rng = np.random.default_rng(7)
    blocks = []
    for p in range(P):
        if p == 2:
            h = nb // 2
            M = sp.block_diag([sp.random(h, h, density=6.0 / h, random_state=rng),
                               sp.random(nb - h, nb - h, density=14.0 / nb, random_state=rng)], format="csr")
        elif p == 1:
            pts = rng.random((nb, 3))
            _, idx = cKDTree(pts).query(pts, k=9)
            M = sp.csr_matrix((rng.random(8 * nb), (np.repeat(np.arange(nb), 8), idx[:, 1:].ravel())), shape=(nb, nb))
        else:
            M = sp.random(nb, nb, density=5.0 / nb, random_state=rng, format="csr")
        blocks.append(M + M.T)
    A = sp.lil_matrix(sp.block_diag(blocks))
    for _ in range(100):
        i, j = rng.integers(0, nb * P, 2)
        A[i, j] = A[j, i] = 0.1
    A = sp.csr_matrix(A)
    A = sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.5))
    A.sort_indices()
    return A, P, (np.arange(nb * P) // nb).astype(np.int32)


def _case(kind, monkeypatch):
    """(A, P, part) of a test problem of test_gpu_configs.py's large-block tests; sets the switches it needs."""
    from oracle import oracle as O
    if kind == "poisson":                                   # slabs of 12 x 24 x 24 = 6912 rows, band 288
        return O.poisson3d(24), 2, None
    if kind == "poisson48":                                 # slabs of 24 x 48 x 48 = 55296 rows, leaves of <= 24 rows:
        monkeypatch.setenv("PREALPS_ND_LEAF", "24")         # > 2048 fronts in the lowest level (many-workgroup kernels)
        monkeypatch.setenv("PREALPS_SETUP_TRACE", "1")
        return O.poisson3d(48), 2, None
    if kind == "chains":                                    # separators cut into 64-column supernodes, small leaves
        monkeypatch.setenv("PREALPS_ND_WIDTH", "64")
        monkeypatch.setenv("PREALPS_ND_LEAF", "24")
        return O.poisson3d(24), 2, None
    if kind == "elasticity":                                # 2 blocks of 14 x 14 x 7 nodes = 4116 rows
        from prealps_amd import gen
        rp, ci, v = gen.elasticity3d_csr(14)
        part, P = gen.box_partition_nodes(14, (14, 14, 7))
        N = len(rp) - 1
        return sp.csr_matrix((v, ci, rp), shape=(N, N)), P, part
    if kind == "random":
        monkeypatch.setenv("PREALPS_BJ_ND", "2")
        return _random_blocks()
    if kind == "mixed":                                     # one sparse block (5600 rows) beside band blocks of 200
        n = 20
        idx = np.arange(n ** 3)
        part = np.where(idx // (n * n) < 14, 0, 1 + (idx - 14 * n * n) // 200).astype(np.int32)
        monkeypatch.setenv("PREALPS_ND_LEAF", "40")
        monkeypatch.setenv("PREALPS_BJ_ND", "2")
        return O.poisson3d(n), int(part.max()) + 1, part
    raise ValueError(kind)


def _ecg_case(kind, monkeypatch):
    """The matrices of _case cut into at least 8 blocks (ECG needs t <= blocks), each with the sparse factor."""
    if kind == "mixed":
        return _case(kind, monkeypatch)
    monkeypatch.setenv("PREALPS_BJ_ND", "2")
    monkeypatch.setenv("PREALPS_BJ_ND_ROWS", "1024")
    if kind == "poisson":                                   # slabs of 3 x 24 x 24 = 1728 rows, band 576
        from oracle import oracle as O
        return O.poisson3d(24), 8, None
    A, P, part = _random_blocks()                           # each random block in two halves of 1300 rows
    return A, 2 * P, (np.arange(A.shape[0]) // (A.shape[0] // (2 * P))).astype(np.int32)


def _problem(A, P, part):
    import prealps_amd
    from oracle import oracle as O
    part = O.contiguous_partition(A.shape[0], P) if part is None else part
    rp, ci, v = O.as_csr(A)
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
    return prob, B, rowpos


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("t", [1, 4, 8, 16])
@pytest.mark.parametrize("kind", ["poisson", "elasticity", "random", "chains", "poisson48"])
def test_single_precision_apply(kind, t, monkeypatch, capfd):
    """Every panel width of the dispatch (2, 4, 8, 16, the one-pass 16-column kernels included), on blocks that all get
    the sparse factor: precision 32, half the factor bytes, and an apply that differs from the fp64 one by fp32
    rounding of the coefficients -- more than 1e-10 (the fp32 copies ran) and less than 1e-6 relative.  Measured
    (MI355X): Poisson 1.09-1.18e-8, elasticity 3.3-3.8e-8, random blocks 8.4-8.5e-9, chains 1.22e-8, Poisson 48^3 1.24-1.31e-8.  The small
    problems run the few-workgroup kernels of every level; "poisson48" has a level of more than 1024 forward and
    2048 backward workgroups (the setup trace says so), i.e. the many-workgroup kernels too."""
    A, P, part = _case(kind, monkeypatch)
    prob, B, rowpos = _problem(A, P, part)
    X = np.random.default_rng(t).standard_normal((prob.m, t))
    try:
        prob.create_block_jacobi(nd_precision="double")
        assert prob.stat("bj_nd_precision") == 64 and prob.stat("bj_nd_blocks") == P
        zd, bytes_d = prob.block_jacobi_apply(X, t), prob.stat("bj_factor_bytes")
        prob.create_block_jacobi(nd_precision="single")
        assert prob.stat("bj_nd_precision") == 32 and prob.stat("bj_nd_blocks") == P
        zs, bytes_s = prob.block_jacobi_apply(X, t), prob.stat("bj_factor_bytes")
    finally:
        prob.close()
    assert bytes_s == bytes_d / 2            # every block has the sparse factor: all of the bytes halve
    d = _rel(zs, zd)
    err = capfd.readouterr().err
    print("%s t=%d: relative difference single / double %.3e" % (kind, t, d))
    assert np.isfinite(zs).all() and 1e-10 < d < 1e-6
    if kind == "poisson48":
        levels = [(int(a), int(b)) for a, b in re.findall(r"(\d+) forward / (\d+) backward workgroups", err)]
        assert max(a for a, b in levels) >= 1024 and max(b for a, b in levels) >= 2048, levels
        assert "[nd] factor stored in single precision" in err


@pytest.mark.parametrize("kind", ["poisson", "random"])
def test_single_precision_factor_is_symmetric_positive_definite(kind, monkeypatch):
    """The backward copy is the exact transpose of the forward one after rounding, so the fp32 block solve is a
    symmetric positive definite operator to fp64 roundoff: y^T M x = x^T M y, x^T M x > 0."""
    A, P, part = _case(kind, monkeypatch)
    prob, B, rowpos = _problem(A, P, part)
    rng = np.random.default_rng(11)
    try:
        prob.create_block_jacobi(nd_precision="single")
        assert prob.stat("bj_nd_precision") == 32
        for _ in range(3):
            X = rng.standard_normal((prob.m, 2))
            Z = prob.block_jacobi_apply(X, 2)
            x, y, mx, my = X[:, 0], X[:, 1], Z[:, 0], Z[:, 1]
            assert abs(y @ mx - x @ my) <= 1e-10 * np.linalg.norm(y) * np.linalg.norm(mx)
            assert x @ mx > 0 and y @ my > 0
    finally:
        prob.close()


@pytest.mark.parametrize("t", [4, 8])
@pytest.mark.parametrize("alg", ["odir", "omin"])
@pytest.mark.parametrize("kind", ["poisson", "random", "mixed"])
def test_ecg_with_single_precision_factor(kind, alg, t, monkeypatch):
    """ECG with the fp32 factor converges to tol; the true residual of x (Finalize) on the permuted, scaled matrix is
    within 2 sqrt(t) tol, and the iteration count within max(2, 3 %) of the oracle's fp64 count.  Poisson and the random
    blocks in 8 sparse blocks; "mixed": one sparse block beside band blocks, so both precisions are live in one apply."""
    import prealps_amd as pa
    from oracle import oracle as O
    ga, oa = {"odir": (pa.ORTHODIR, O.ORTHODIR), "omin": (pa.ORTHOMIN, O.ORTHOMIN)}[alg]
    A, P, part = _ecg_case(kind, monkeypatch)
    prob, B, rowpos = _problem(A, P, part)
    tol = 1e-5
    try:
        prob.create_block_jacobi(nd_precision="single")
        assert prob.stat("bj_nd_precision") == 32 and prob.stat("bj_nd_blocks") == (1 if kind == "mixed" else P)
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, t, ortho_alg=ga, tol=tol)
    finally:
        prob.close()
    ref = O.ECG(B, rowpos, t, ortho_alg=oa, tol=tol).solve(rhs)
    true_res = float(np.linalg.norm(rhs - B @ got.x) / np.linalg.norm(rhs))
    print("%s %s t=%d: %d iterations (fp64 oracle %d), true residual %.3e" % (kind, alg, t, got.iters, ref["iters"], true_res))
    assert got.iters < 1000
    assert true_res <= 2.0 * np.sqrt(t) * tol
    assert abs(got.iters - ref["iters"]) <= max(2, 0.03 * ref["iters"])


def test_default_is_fp64_bit_for_bit(monkeypatch):
    """Unset, the sparse factor is fp64 and the apply has the bits of PREALPS_BJ_ND_PRECISION=double;
    preAlps_hip_set_nd_precision(64) overrides PREALPS_BJ_ND_PRECISION=single, and 0 follows it again."""
    from prealps_amd.lib import check
    A, P, part = _case("poisson", monkeypatch)
    prob, B, rowpos = _problem(A, P, part)
    X = np.random.default_rng(3).standard_normal((prob.m, 4))
    L = prob.L
    try:
        monkeypatch.delenv(SW, raising=False)
        prob.create_block_jacobi()
        assert prob.stat("bj_nd_precision") == 64
        z_unset = prob.block_jacobi_apply(X, 4)
        monkeypatch.setenv(SW, "double")
        prob.create_block_jacobi()
        assert prob.stat("bj_nd_precision") == 64
        assert _same_bits(prob.block_jacobi_apply(X, 4), z_unset)
        monkeypatch.setenv(SW, "single")
        check(L.preAlps_hip_set_nd_precision(64), "preAlps_hip_set_nd_precision")
        try:
            prob.create_block_jacobi()
            assert prob.stat("bj_nd_precision") == 64
            assert _same_bits(prob.block_jacobi_apply(X, 4), z_unset)
        finally:
            L.preAlps_hip_set_nd_precision(0)
        prob.create_block_jacobi()
        assert prob.stat("bj_nd_precision") == 32
        assert not _same_bits(prob.block_jacobi_apply(X, 4), z_unset)
    finally:
        prob.close()


def test_switch_changes_nothing_without_sparse_blocks(monkeypatch):
    """Blocks of 1728 rows get the band factor: the switch leaves them in fp64 (precision stat 0, same bits)."""
    from oracle import oracle as O
    prob, B, rowpos = _problem(O.poisson3d(24), 8, None)
    X = np.random.default_rng(5).standard_normal((prob.m, 4))
    out = {}
    try:
        for v in ("double", "single"):
            monkeypatch.setenv(SW, v)
            prob.create_block_jacobi()
            assert prob.stat("bj_nd_blocks") == 0 and prob.stat("bj_nd_precision") == 0
            out[v] = prob.block_jacobi_apply(X, 4)
    finally:
        prob.close()
    assert _same_bits(out["single"], out["double"])


def test_host_numeric_path_rounds_the_same_factor(monkeypatch):
    """PREALPS_ND_NUMERIC=host rounds the pair it uploads: the same fp32 apply as the device path to 1e-6 (the fp64
    panels of the two paths differ by roundoff, so a few entries round to a neighbouring float)."""
    A, P, part = _case("poisson", monkeypatch)
    X = np.random.default_rng(9).standard_normal((A.shape[0], 4))
    out = {}
    for numeric in ("device", "host"):
        monkeypatch.setenv("PREALPS_ND_NUMERIC", numeric)
        prob, B, rowpos = _problem(A, P, part)
        try:
            prob.create_block_jacobi(nd_precision="single")
            assert prob.stat("bj_nd_precision") == 32
            out[numeric] = prob.block_jacobi_apply(X, 4)
        finally:
            prob.close()
    assert _rel(out["host"], out["device"]) <= 1e-6


def test_bad_value_fails_create(monkeypatch):
    """PREALPS_BJ_ND_PRECISION=half: create fails (return-code mode) and names the switch; the Python keyword refuses
    unknown values; a non-zero preAlps_hip_set_nd_precision does not read the switch at all."""
    import prealps_amd as pa
    A, P, part = _case("poisson", monkeypatch)
    monkeypatch.setenv(SW, "half")
    prob, B, rowpos = _problem(A, P, part)
    try:
        with pytest.raises(pa.PreAlpsError, match=SW):
            prob.create_block_jacobi()
        with pytest.raises(ValueError):
            prob.create_block_jacobi(nd_precision="half")
        prob.create_block_jacobi(nd_precision="single")
        assert prob.stat("bj_nd_precision") == 32
    finally:
        prob.close()
