"""preAlps_BlockJacobiUpdateValues on the device: after new values for the same pattern and a numeric refactorisation
in place, the block solve has the bits of a fresh create from those values -- through k_bj_factor and k_bj_factor_big,
one-copy (fp64 / fp32) and paired records, window-slot and narrow records, mixed classes, a shard with halo columns --
at the same device addresses, with one band map per create; blocks with the sparse factor are created again beside
band blocks refreshed in place; refusals leave the factor alone; values that are not SPD leave no preconditioner."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ENTRY = "preAlps_BlockJacobiUpdateValues"


def _new_values(rp, ci, v):
    """v2 = S A S, S = diag(1 + 0.3 (2u - 1)): the pattern stays, the matrix stays SPD, every value and the scaling
    vector change."""
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    rows = np.repeat(np.arange(N), np.diff(rp))
    return s[rows] * v * s[ci]


def _two_cubes(n):
    """Two cubes of n^3 Poisson nodes, one block each (test_gpu_configs.py::test_block_solve_dispatch_by_band)."""
    T = sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    T2 = sp.diags([-np.ones(2 * n - 1), 2 * np.ones(2 * n), -np.ones(2 * n - 1)], [-1, 0, 1])
    I, I2 = sp.identity(n), sp.identity(2 * n)
    return sp.csr_matrix(sp.kron(sp.kron(T2, I), I) + sp.kron(sp.kron(I2, T), I) + sp.kron(sp.kron(I2, I), T))


# (rows, band) per block: 1 .. 192 rows at bands 0 .. 64 in one launch; 256 rows, the last index of the packed row map,
# at bands 40 and 112 beside small blocks; band 129 (default dispatch: one workgroup per block, k_bj_factor_big)
BAND_BLOCKS = {
    "band-mixed": [(b, w) for w in (64, 0, 33, 5, 32) for b in (1, 192, 2, 129, 3, 128, 4, 127, 5, 65, 15, 64, 16, 63, 17, 191)],
    "band-256": 2 * [(256, 40), (1, 0), (130, 112), (256, 112), (16, 40), (130, 40), (2, 1)],
    "band-129": [(192, 129), (130, 129), (300, 129), (500, 129)],
}


@functools.lru_cache(maxsize=None)
def _matrix(kind):
    """rowptr, colind, val, val2, number of parts, partition vector."""
    from oracle import oracle as O
    from prealps_amd import gen
    if kind.startswith("boxes"):                      # Poisson n^3 in boxes
        n, box = {"boxes20": (20, (5, 5, 10)), "boxes24": (24, (4, 4, 12)), "boxes10": (10, (5, 5, 5))}[kind]
        rp, ci, v = gen.poisson3d_csr(n)
        part, P = gen.box_partition(n, box)
    elif kind.startswith("cubes"):
        A = _two_cubes(int(kind[5:]))
        rp, ci, v = O.as_csr(A)
        P, part = 2, O.contiguous_partition(A.shape[0], 2)
    elif kind == "elasticity12":
        nn = (12, 10, 10)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, P = gen.box_partition_nodes(nn, (2, 2, 2))
    elif kind == "poisson12":                         # 5 contiguous parts (the shard: parts 1 and 2 of them)
        A = O.poisson3d(12)
        rp, ci, v = O.as_csr(A)
        P, part = 5, O.contiguous_partition(A.shape[0], 5)
    elif kind == "poisson12-mixed":                   # one part of 864 rows, six of 144
        rp, ci, v = O.as_csr(O.poisson3d(12))
        P, part = 7, np.concatenate([np.zeros(864, dtype=np.int32), np.repeat(np.arange(1, 7, dtype=np.int32), 144)])
    elif kind in BAND_BLOCKS:                         # synthetic blocks with prescribed rows and a full band
        rp, ci, v, part, P = gen.band_blocks_csr(BAND_BLOCKS[kind], seed=len(kind), grading=2.0)
    else:
        raise KeyError(kind)
    return rp, ci, v, _new_values(rp, ci, v), P, part


def _problem(rp, ci, v, P, part, **kw):
    import prealps_amd
    return prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _addresses(prob):
    return prob.stat("bj_records_address"), prob.stat("bj_g4_address")


def _fresh_apply(kind, X, t, create_kw=None, **kw):
    rp, ci, v, v2, P, part = _matrix(kind)
    fresh = _problem(rp, ci, v2, P, part, **kw)
    try:
        fresh.create_block_jacobi(**(create_kw or {}))
        return fresh.block_jacobi_apply(X, t)
    finally:
        fresh.close()


def _check_refreshed(prob, at):
    assert _addresses(prob) == at and at[0] != 0
    assert prob.stat("bj_values_epoch") == prob.stat("op_values_epoch")
    assert prob.stat("bj_band_map_builds") == 1


def _refactor_case(kind, t, create_kw=None, **kw):
    """Create on v, update to v2, refactor in place: the apply against a fresh create on v2, in bits."""
    rp, ci, v, v2, P, part = _matrix(kind)
    prob = _problem(rp, ci, v, P, part, **kw)
    try:
        X = np.random.default_rng(t).standard_normal((prob.m, t))
        prob.create_block_jacobi(**(create_kw or {}))
        Z0 = prob.block_jacobi_apply(X, t)
        at = _addresses(prob)
        assert prob.stat("bj_band_map_builds") == 0 and prob.stat("bj_band_map_bytes") == 0 and prob.stat("bj_updates") == 0
        prob.update_values(v2)
        assert prob.stat("bj_values_epoch") < prob.stat("op_values_epoch")
        prob.refactor_block_jacobi()
        _check_refreshed(prob, at)
        assert prob.stat("bj_updates") == 1 and prob.stat("bj_update_nd_rebuilt") == 0
        assert prob.stat("bj_band_map_bytes") >= 8 * prob.stat("bj_band_map_entries") > 0
        Z1 = prob.block_jacobi_apply(X, t)
        stats = {k: prob.stat(k) for k in ("bj_max_bandwidth", "bj_g4_bytes", "bj_pairs_bytes", "bj_band_precision",
                                           "bj_band_map_entries", "bj_band_map_bytes", "bj_factor_bytes")}
    finally:
        prob.close()
    Zf = _fresh_apply(kind, X, t, create_kw, **kw)
    print("%s t=%d: %s" % (kind, t, stats))
    assert _same_bits(Z1, Zf)
    assert not np.array_equal(Z1, Z0)
    return stats


# ---- k_bj_factor: one-copy and paired records --------------------------------------------------------------
@pytest.mark.parametrize("t", [4, 8, 16])
@pytest.mark.parametrize("kind", ["boxes20", "boxes24"])
def test_narrow_bands_have_the_bits_of_a_fresh_create(kind, t, monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    stats = _refactor_case(kind, t)
    assert stats["bj_g4_bytes"] > 0 and stats["bj_band_precision"] == 64


@pytest.mark.parametrize("kind", ["boxes20", "boxes24"])
def test_paired_records_without_the_one_copy_records(kind, monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    monkeypatch.setenv("PREALPS_BJ_G4", "0")
    stats = _refactor_case(kind, 4)
    assert stats["bj_g4_bytes"] == 0 and stats["bj_pairs_bytes"] > 0


def test_single_precision_one_copy_records(monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    stats = _refactor_case("boxes20", 4, create_kw={"band_precision": "single"})
    assert stats["bj_band_precision"] == 32


# ---- k_bj_factor_big ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_from", ["default", "448"])
def test_blocked_factorisation_window_slot_and_narrow_records(wide_from, monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_ND", "0")
    if wide_from != "default":
        monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", wide_from)
    stats = _refactor_case("cubes14", 4)
    assert 129 <= stats["bj_max_bandwidth"] <= 192


def test_two_cubes_of_eight_at_eight_columns(monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_ND", "0")
    stats = _refactor_case("cubes8", 8)
    assert 49 <= stats["bj_max_bandwidth"] <= 80


# ---- mixed classes, scaling; a shard --------------------------------------------------------------------------
def test_elasticity_boxes_mixed_classes():
    _refactor_case("elasticity12", 4)


def test_a_shard_with_halo_columns():
    """Rank 1 of 3 rehearsed in this process (preAlps_hip_loopback): the panel's columns reach outside its rows."""
    import prealps_amd
    L = prealps_amd.load()
    try:
        _refactor_case("poisson12", 4, shard=(1, 3))
    finally:                                              # one process, no hooks, for the tests that follow
        L.preAlps_hip_set_world(0, 1)
        L.preAlps_hip_set_comm(prealps_amd.lib.ALLREDUCE_FN(), prealps_amd.lib.EXCHANGE_FN(), None)


# ---- synthetic band blocks: unequal rows in one class, 256 rows, just outside the one-copy records ------------------
@pytest.mark.parametrize("t", [4, 8, 16])
@pytest.mark.parametrize("kind", ["band-mixed", "band-256"])
def test_unequal_band_blocks_have_the_bits_of_a_fresh_create(kind, t, monkeypatch):
    """k_bj_band_assemble and k_bj_factor writing into old records of blocks of 1 .. 192 (256) rows side by side."""
    monkeypatch.setenv("PREALPS_BJ_ND", "0")
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    stats = _refactor_case(kind, t)
    assert stats["bj_max_bandwidth"] == max(min(w, b - 1) for b, w in BAND_BLOCKS[kind])
    assert stats["bj_g4_bytes"] > 0 and stats["bj_pairs_bytes"] == 0 and stats["bj_band_precision"] == 64


@pytest.mark.parametrize("kind", ["band-mixed", "band-256"])
def test_unequal_band_blocks_with_single_precision_records(kind, monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_ND", "0")
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    stats = _refactor_case(kind, 4, create_kw={"band_precision": "single"})
    assert stats["bj_band_precision"] == 32


@pytest.mark.parametrize("t", [4, 8])
def test_band_129_just_outside_the_one_copy_records(t, monkeypatch):
    """Default dispatch, few blocks: band 129 has window-slot records, k_bj_factor_big and k_bj_layout_big refresh them."""
    monkeypatch.setenv("PREALPS_BJ_ND", "0")
    stats = _refactor_case("band-129", t)
    assert stats["bj_max_bandwidth"] == 129 and stats["bj_g4_bytes"] == 0 and stats["bj_pairs_bytes"] == 0


# ---- the map is cut once ----------------------------------------------------------------------------------------
def test_the_map_is_reused_and_an_update_can_be_undone(monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    rp, ci, v, v2, P, part = _matrix("boxes20")
    X = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi()
        Z0 = prob.block_jacobi_apply(X, 4)
        at = _addresses(prob)
        prob.update_values(v2)
        prob.refactor_block_jacobi()
        _check_refreshed(prob, at)
        Z1 = prob.block_jacobi_apply(X, 4)
        prob.update_values(v, precond="refactor")
        _check_refreshed(prob, at)
        assert prob.stat("bj_updates") == 2 and prob.stat("op_values_epoch") == 2
        Z2 = prob.block_jacobi_apply(X, 4)
    finally:
        prob.close()
    assert _same_bits(Z2, Z0) and not np.array_equal(Z1, Z0)


# ---- solve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["boxes10", "elasticity12"])
def test_solve_after_an_update_with_the_factor_refreshed_in_place(kind):
    import prealps_amd as pa
    rp, ci, v, v2, P, part = _matrix(kind)
    t = 4
    prob = _problem(rp, ci, v, P, part)
    try:
        rhs = prob.reference_rhs()
        old = prob.solve(rhs, t, ortho_alg=pa.ORTHODIR, tol=1e-5)     # plan and factor of the old values are in use
        at = _addresses(prob)
        prob.update_values(v2, precond="refactor")
        _check_refreshed(prob, at)
        assert prob.stat("bj_values_epoch") == prob.stat("op_values_epoch") == 1
        got = prob.solve(rhs, t, ortho_alg=pa.ORTHODIR, tol=1e-5)
    finally:
        prob.close()
    fresh = _problem(rp, ci, v2, P, part)
    try:
        ref = fresh.solve(rhs, t, ortho_alg=pa.ORTHODIR, tol=1e-5)
    finally:
        fresh.close()
    assert got.iters == ref.iters and 0 < got.iters < 1000
    assert _same_bits(got.res, ref.res) and _same_bits(got.x, ref.x)
    assert not np.array_equal(got.x, old.x)


# ---- sparse-factored blocks beside band blocks ---------------------------------------------------------------------
def test_sparse_blocks_are_created_again_beside_band_blocks(monkeypatch):
    from oracle import oracle as O
    monkeypatch.setenv("PREALPS_BJ_ND", "2")
    monkeypatch.setenv("PREALPS_BJ_ND_ROWS", "512")
    rp, ci, v, v2, P, part = _matrix("poisson12-mixed")
    N, t = len(rp) - 1, 4
    X = np.random.default_rng(t).standard_normal((N, t))
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi()
        assert prob.stat("bj_nd_blocks") == 1
        Z0 = prob.block_jacobi_apply(X, t)
        at = _addresses(prob)
        prob.update_values(v2)
        prob.refactor_block_jacobi()
        _check_refreshed(prob, at)
        assert prob.stat("bj_update_nd_rebuilt") == 1 and prob.stat("bj_nd_blocks") == 1
        Z1 = prob.block_jacobi_apply(X, t)
    finally:
        prob.close()
    Zf = _fresh_apply("poisson12-mixed", X, t)
    band = slice(864, N)                                  # (a contiguous partition: the panel keeps the row order)
    assert _same_bits(Z1[band], Zf[band]) and not np.array_equal(Z1[band], Z0[band])
    print("rows of the sparse-factored block match the fresh create in bits: %s" % _same_bits(Z1[:864], Zf[:864]))
    A2 = sp.csr_matrix((v2, ci, rp), shape=(N, N))
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(A2), part, P)
    zr = O.BlockJacobi(B, rowpos).apply(X)
    np.testing.assert_allclose(Z1, zr, rtol=1e-9, atol=1e-9 * np.abs(zr).max())


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refused_without_a_preconditioner():
    import prealps_amd
    rp, ci, v, v2, P, part = _matrix("boxes10")
    prob = _problem(rp, ci, v, P, part)
    try:
        with pytest.raises(prealps_amd.PreAlpsError, match=ENTRY + ".*not created"):
            prob.refactor_block_jacobi()
        prob.update_values(v2, precond="refactor")        # no preconditioner: the operator alone, as "rebuild" does
        assert prob.stat("op_values_epoch") == 1 and not prob.has_precond
    finally:
        prob.close()


def test_refused_for_a_host_factored_preconditioner(monkeypatch):
    import prealps_amd
    monkeypatch.setenv("PREALPS_BJ_FACTOR", "host")
    rp, ci, v, v2, P, part = _matrix("boxes10")
    X = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi()
        Z0 = prob.block_jacobi_apply(X, 4)
        prob.update_values(v2)
        monkeypatch.delenv("PREALPS_BJ_FACTOR")           # the create's decision counts, not the switch of today
        with pytest.raises(prealps_amd.PreAlpsError, match=ENTRY + ".*free and create instead"):
            prob.refactor_block_jacobi()
        assert prob.has_precond and prob.stat("bj_updates") == 0 and prob.stat("bj_band_map_builds") == 0
        assert prob.stat("bj_values_epoch") < prob.stat("op_values_epoch")
        assert _same_bits(prob.block_jacobi_apply(X, 4), Z0)
    finally:
        prob.close()


def test_refused_after_the_operator_was_built_again():
    import prealps_amd
    rp, ci, v, v2, P, part = _matrix("boxes10")
    X = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi()
        Z0 = prob.block_jacobi_apply(X, 4)
        again = _problem(rp, ci, v2, P, part)             # the library's one operator is built again; the factor stays
        with pytest.raises(prealps_amd.PreAlpsError, match=ENTRY + ".*built again"):
            prob.refactor_block_jacobi()
        assert prob.has_precond and prob.stat("bj_updates") == 0
        assert _same_bits(prob.block_jacobi_apply(X, 4), Z0)
        again.close()
    finally:
        prob.close()


# ---- values that are not SPD ---------------------------------------------------------------------------------------
def test_values_that_are_not_spd_leave_no_preconditioner():
    import re
    import prealps_amd
    rp, ci, v, v2, P, part = _matrix("boxes10")
    N = len(rp) - 1
    X = np.random.default_rng(4).standard_normal((N, 4))
    bad_row = N // 2
    k = rp[bad_row] + int(np.flatnonzero(ci[rp[bad_row]:rp[bad_row + 1]] == bad_row)[0])
    v3 = v2.copy()
    v3[k] = -v3[k]
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi()
        prob.block_jacobi_apply(X, 4)
        with pytest.raises(prealps_amd.PreAlpsError, match=ENTRY) as err:
            prob.update_values(v3, precond="refactor")
        m = re.search(r"not SPD \(global row (\d+)\)", str(err.value))
        assert m, str(err.value)
        assert prob.perm[int(m.group(1))] == bad_row
        assert not prob.has_precond
        dx, dy = prob.panel(4, 4), prob.panel(4, 4)
        try:
            assert prob.L.preAlps_BlockJacobiApply(C.byref(dx), C.byref(dy)) != 0
            assert b"preconditioner not created" in prob.L.preAlps_hip_last_error()
        finally:
            prob.panel_free(dx)
            prob.panel_free(dy)
        prob.update_values(v2, precond="rebuild")         # SPD values again; the next apply creates the factor
        Z = prob.block_jacobi_apply(X, 4)
        assert prob.has_precond and prob.stat("bj_values_epoch") == prob.stat("op_values_epoch") == 2
    finally:
        prob.close()
    assert _same_bits(Z, _fresh_apply("boxes10", X, 4))
