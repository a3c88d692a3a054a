"""Identical diagonal blocks read one shared factor record (prealps_amd/csrc/bj_share.c, the read offsets of
block_jacobi.c, k_bj_share_check of bj_refactor.hip).  Every case creates the same problem twice in one process, with
PREALPS_BJ_SHARE=0 and with the switch unset, and applies both preconditioners to the same random panels of 1, 3, 4 and
8 columns: Z must be the same bytes, and sharing must really have happened -- bj_shared_blocks is at least what a numpy
restatement counts on the natural-order in-block entries under the library's scaling rule (sqrt(1 / max_j |a_ij|) per
row, pa_op_scaling); at least, because the factor order may merge classes that the natural order keeps apart."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

COLS = (1, 3, 4, 8)


def _problem(rp, ci, v, P, part):
    import prealps_amd
    return prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _natural_classes(rp, ci, v, part, P):
    """first[p]: the lowest-numbered part whose diagonal block, scaled as the library scales it and in the given row
    order, has the same rows and the same entries (local row, local column, value bits) as part p's."""
    rp, ci, v, part = np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(v, np.float64), np.asarray(part, np.int64)
    N = len(rp) - 1
    rows = np.repeat(np.arange(N), np.diff(rp))
    d = np.sqrt(1.0 / np.maximum.reduceat(np.abs(v), rp[:-1]))
    sv = (d[rows] * v) * d[ci]
    order = np.argsort(part, kind="stable")
    rowpos = np.concatenate([[0], np.cumsum(np.bincount(part, minlength=P))])
    loc = np.empty(N, np.int64)
    loc[order] = np.arange(N) - rowpos[part[order]]
    inb = part[rows] == part[ci]
    seen, first = {}, []
    for p in range(P):
        sel = inb & (part[rows] == p)
        key = (int(rowpos[p + 1] - rowpos[p]), loc[rows[sel]].tobytes(), loc[ci[sel]].tobytes(), sv[sel].tobytes())
        first.append(seen.setdefault(key, p))
    return np.asarray(first)


def _expected_shared(rp, ci, v, part, P):
    return int(np.count_nonzero(_natural_classes(rp, ci, v, part, P) != np.arange(P)))


def _band_copies():
    """Block-diagonal matrix of random SPD band blocks at the dispatch edges: per shape (b rows, band w) the sequence
    A, D, A, D, A with D = A but for the last bit of one value (and of its mirror)."""
    rng = np.random.default_rng(20261020)
    mats = []
    for b in (1, 5, 16, 17, 192, 256):
        for w in (0, 33, 64):
            if w >= b:
                continue
            i, j = np.indices((b, b))
            L0 = np.where((i - j <= w) & (i > j), rng.uniform(0.25, 1.0, (b, b)) * rng.choice([-1.0, 1.0], (b, b)) / np.sqrt(w + 1.0), 0.0)
            L0 += np.diag(rng.uniform(1.0, 2.0, b))
            A = L0 @ L0.T
            A = np.tril(A) + np.tril(A, -1).T
            D = A.copy()
            r, c = (b - 1, b - 1 - w // 2)                    # an in-band entry (the last diagonal entry when w = 0)
            x = D[r:r + 1, c:c + 1].view(np.uint64)
            x ^= np.uint64(1)
            D[c, r] = D[r, c]
            assert D.tobytes() != A.tobytes() and np.array_equal(D, D.T)
            mats += [sp.csr_matrix(M) for M in (A, D, A, D, A)]
    M = sp.block_diag(mats, format="csr")
    M.sort_indices()
    part = np.repeat(np.arange(len(mats)), [m.shape[0] for m in mats]).astype(np.int32)
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64), len(mats), part


@functools.lru_cache(maxsize=None)
def _matrix(kind):
    from prealps_amd import gen
    if kind == "poisson12":
        rp, ci, v = gen.poisson3d_csr(12)
        part, P = gen.box_partition(12, (5, 5, 10))
    elif kind == "elasticity":
        nn = (10, 16, 32)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, P = gen.box_partition_nodes(nn, (2, 4, 8))
    elif kind == "band-copies":
        rp, ci, v, P, part = _band_copies()
    else:
        raise KeyError(kind)
    return rp, ci, v, P, part


def _panels(m):
    return {t: np.random.default_rng(100 + t).standard_normal((m, t)) for t in COLS}


def _create_and_apply(rp, ci, v, P, part, create_kw=None):
    """Z for every panel, and the share stats, of a fresh create under the current environment"""
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi(**(create_kw or {}))
        X = _panels(prob.m)
        Z = {t: prob.block_jacobi_apply(X[t], t) for t in COLS}
        stats = {k: prob.stat(k) for k in ("bj_share_classes", "bj_shared_blocks", "bj_share_distinct_g4_bytes", "bj_g4_bytes",
                                           "bj_band_precision", "bj_parts_local")}
    finally:
        prob.close()
    return Z, stats


def _share_case(kind, monkeypatch, create_kw=None):
    rp, ci, v, P, part = _matrix(kind)
    monkeypatch.setenv("PREALPS_BJ_SHARE", "0")
    Z0, s0 = _create_and_apply(rp, ci, v, P, part, create_kw)
    monkeypatch.delenv("PREALPS_BJ_SHARE")
    Z1, s1 = _create_and_apply(rp, ci, v, P, part, create_kw)
    want = _expected_shared(rp, ci, v, part, P)
    print("%s: %d blocks, expected shared >= %d, got %d in %d classes; one-copy records %.0f bytes, read %.0f"
          % (kind, P, want, s1["bj_shared_blocks"], s1["bj_share_classes"], s1["bj_g4_bytes"], s1["bj_share_distinct_g4_bytes"]))
    # PREALPS_BJ_SHARE=0: every block reads its own records
    assert s0["bj_shared_blocks"] == 0 and s0["bj_share_classes"] == P == s0["bj_parts_local"]
    assert s0["bj_share_distinct_g4_bytes"] == s0["bj_g4_bytes"] == s1["bj_g4_bytes"]
    for t in COLS:
        assert _same_bits(Z0[t], Z1[t]), (kind, t)
        assert np.isfinite(Z1[t]).all() and np.abs(Z1[t]).max() > 0
    assert want > 0 and s1["bj_shared_blocks"] >= want
    assert s1["bj_share_classes"] == P - s1["bj_shared_blocks"]
    assert 0 < s1["bj_share_distinct_g4_bytes"] < s1["bj_g4_bytes"]
    return s1, want


def test_poisson_boxes_read_one_record_per_box_shape(monkeypatch):
    """Poisson 12^3 in boxes of 5 x 5 x 10: 18 blocks of six sizes."""
    s, want = _share_case("poisson12", monkeypatch)
    assert s["bj_band_precision"] == 64


def test_elasticity_boxes_mixed_classes(monkeypatch):
    """Elasticity on (10, 16, 32) nodes in boxes of 2 x 4 x 8: 80 blocks, the coefficient jumps and the bottom layer
    make blocks of the same shape differ."""
    _share_case("elasticity", monkeypatch)


def test_band_blocks_at_the_dispatch_edges_apart_by_one_bit(monkeypatch):
    """Rows 1 .. 256, bands 0 .. 64: three copies of a block interleaved with two of a block that differs in the last
    bit of one value.  At least the banded shapes must keep A and D apart after the scaling (the restatement says
    which do): a D that read A's records would show in Z."""
    rp, ci, v, P, part = _matrix("band-copies")
    first = _natural_classes(rp, ci, v, part, P)
    apart = sum(int(first[q + 1] != first[q]) for q in range(0, P, 5))
    assert apart >= 6                                       # (8 of the 10 shapes; the scaling rounds two diagonal shapes together)
    _share_case("band-copies", monkeypatch)


def test_single_precision_records(monkeypatch):
    s, _ = _share_case("poisson12", monkeypatch, create_kw={"band_precision": "single"})
    assert s["bj_band_precision"] == 32


def test_a_refresh_keeps_the_classes_that_survive_and_splits_the_others():
    """New values on Poisson 12^3: all values doubled -- every class survives; then one in-block entry (and its mirror)
    of a block that reads another block's records halved -- that block reads its own again.  Z has the bits of a
    fresh create from the same values both times."""
    rp, ci, v, P, part = _matrix("poisson12")
    first = _natural_classes(rp, ci, v, part, P)
    p = int(np.nonzero(first != np.arange(P))[0][0])          # a block that repeats an earlier one
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    e = int(np.nonzero((part[rows] == p) & (part[ci] == p) & (rows < ci))[0][0])
    i, j = int(rows[e]), int(ci[e])
    v2 = 2.0 * v
    v3 = v2.copy()
    v3[e] *= 0.5
    v3[np.nonzero((rows == j) & (ci == i))[0][0]] *= 0.5
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi()
        X = _panels(prob.m)
        shared0, classes0 = prob.stat("bj_shared_blocks"), prob.stat("bj_share_classes")
        read0 = prob.stat("bj_share_distinct_g4_bytes")
        prob.update_values(v2, precond="refactor")
        shared2, Z2 = prob.stat("bj_shared_blocks"), {t: prob.block_jacobi_apply(X[t], t) for t in COLS}
        prob.update_values(v3, precond="refactor")
        shared3, Z3 = prob.stat("bj_shared_blocks"), {t: prob.block_jacobi_apply(X[t], t) for t in COLS}
        read3 = prob.stat("bj_share_distinct_g4_bytes")
        assert prob.stat("bj_share_classes") == classes0     # (the create's count: rep itself is not changed)
        prob.update_values(v2, precond="refactor")            # back: the block shares again
        shared4, Z4 = prob.stat("bj_shared_blocks"), {t: prob.block_jacobi_apply(X[t], t) for t in COLS}
    finally:
        prob.close()
    print("shared blocks: create %d, doubled %d, one entry halved %d, doubled again %d" % (shared0, shared2, shared3, shared4))
    F2, s2 = _create_and_apply(rp, ci, v2, P, part)
    F3, s3 = _create_and_apply(rp, ci, v3, P, part)
    assert shared0 >= _expected_shared(rp, ci, v, part, P) > 0
    assert shared2 == shared0 == shared4 == s2["bj_shared_blocks"]
    assert shared3 <= shared0 - 1 and read3 > read0
    for t in COLS:
        assert _same_bits(Z2[t], F2[t]) and _same_bits(Z3[t], F3[t]) and _same_bits(Z4[t], F2[t]), t
        assert not np.array_equal(Z3[t], Z2[t])
