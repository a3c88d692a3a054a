"""The run plan's values on the device without their stored +0.0 entries (PREALPS_SPMM_PACK, spmm_pack.h): the packed
kernels execute the same FMAs in the same order on the same bits, so every product, residual history and solution has
the bits of the unpacked plan's; an update of the values writes through the pack or packs anew; and the default packs
where it takes a tenth off the stream (Q1 elasticity) and nowhere else (Poisson).

Against scipy the products are held to rtol 1e-12 the way test_gpu_parity.py holds them (atol = 1e-12 max |Yref|), and
to |Y - Yref| <= 1e-12 (|A| |X|) entry by entry -- a relative tolerance of 1e-12 on the terms of the sum, which an
entry that cancels to a small value still meets.

Blocks: pa_spmm_plan_build gives a workgroup at most four slices (256 / 64 rows), so no plan has a block of more than
four; the case with the most slices per block that the builder cuts -- "ragged" of spmm_block_cases.py, blocks of four
slices of 1 .. 64 rows across subdomains, every wavefront of a workgroup at work -- stands in for it."""
import numpy as np
import pytest
import scipy.sparse as sp

import spmm_block_cases as S

pytestmark = pytest.mark.gpu

_SWITCHES = ("PREALPS_SPMM_STAGED", "PREALPS_SPMM_RUNS", "PREALPS_SPMM_PACK", "PREALPS_SPMM_GRAM")


def _env(monkeypatch, **env):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _random_spd(n, density, seed):       # (test_gpu_parity.py)
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=rng, format="csr")
    A = M + M.T
    A = A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def _matrix(kind):
    """rowptr, colind, val, parts, partition vector."""
    from oracle import oracle as O
    from prealps_amd import gen
    if kind == "elasticity7":
        rp, ci, v = gen.elasticity3d_csr(7)
        return rp, ci, v, 8, O.contiguous_partition(len(rp) - 1, 8)
    if kind == "elasticity9":
        rp, ci, v = gen.elasticity3d_csr(9)
        part, P = gen.box_partition_nodes(9, (3, 3, 3))
        return rp, ci, v, P, part
    if kind == "elasticity12":
        nn = (12, 10, 10)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, P = gen.box_partition_nodes(nn, (2, 2, 2))
        return rp, ci, v, P, part
    if kind == "random":
        rp, ci, v = O.as_csr(_random_spd(1500, 0.004, 11))
        return rp, ci, v, 7, O.contiguous_partition(len(rp) - 1, 7)
    if kind == "poisson12":
        A = O.poisson3d(12)
        rp, ci, v = O.as_csr(A)
        return rp, ci, v, 5, O.contiguous_partition(A.shape[0], 5)
    if kind == "ragged":
        rp, ci, v = S.matrix("ragged")
        part, P, _ = S.partition("ragged")
        return rp, ci, v, P, part
    raise KeyError(kind)


def _problem(rp, ci, v, P, part, **kw):
    import prealps_amd
    return prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0, **kw)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _product(monkeypatch, mat, t, pack, seed, env=None, reference=True, **kw):
    """Y = A X through a fresh operator with PREALPS_SPMM_PACK = pack (None: unset), its statistics, and the row-wise
    scale |A| |X| with scipy's product of the operator's own panel."""
    _env(monkeypatch, **dict(env or {}, **({} if pack is None else {"PREALPS_SPMM_PACK": pack})))
    prob = _problem(*mat, **kw)
    try:
        X = np.random.default_rng(seed).standard_normal((prob.m, t))
        Y = prob.block_operator(X, t)
        stats = {k: prob.stat(k) for k in ("spmm_packed", "spmm_runs", "spmm_packed_values", "spmm_packed_stream_bytes",
                                           "spmm_stream_bytes", "spmm_stored_entries", "halo_rows")}
        ref = None
        if reference:
            rp, ci, v = prob.local_csr()
            A = sp.csr_matrix((v, ci, rp), shape=(prob.m, max(prob.m, int(ci.max()) + 1)))
            if A.shape[1] == prob.m:
                ref = (A @ X, abs(A) @ np.abs(X))
    finally:
        prob.close()
    return Y, stats, ref


_PRODUCTS = {
    "elasticity7-t1": ("elasticity7", 1, {}, {}),
    "elasticity7-t2": ("elasticity7", 2, {}, {}),
    "elasticity7-t4": ("elasticity7", 4, {}, {}),
    "elasticity12-t4": ("elasticity12", 4, {}, {}),
    "random-forced-runs-t4": ("random", 4, {"PREALPS_SPMM_RUNS": "2"}, {}),
    "ragged-blocks-of-four-t4": ("ragged", 4, {"PREALPS_SPMM_RUNS": "2"}, {}),
}


@pytest.mark.parametrize("case", list(_PRODUCTS))
def test_packed_products_have_the_bits_of_the_unpacked_plan(case, monkeypatch):
    kind, t, env, kw = _PRODUCTS[case]
    mat = _matrix(kind)
    Y1, s1, ref = _product(monkeypatch, mat, t, 1, 7, env, **kw)
    Y0, s0, _ = _product(monkeypatch, mat, t, 0, 7, env, reference=False, **kw)
    print("%s: %d of %d stored values kept, stream %.0f -> %.0f bytes" % (
        case, s1["spmm_packed_values"], s1["spmm_stored_entries"], s1["spmm_stream_bytes"], s1["spmm_packed_stream_bytes"]))
    assert s1["spmm_packed"] == 1 and s1["spmm_runs"] == 1 and s0["spmm_packed"] == 0 and s0["spmm_runs"] == 1
    assert s0["spmm_packed_values"] == 0 and s0["spmm_packed_stream_bytes"] == 0
    assert 0 < s1["spmm_packed_values"] <= s1["spmm_stored_entries"]
    assert s1["spmm_stream_bytes"] == s0["spmm_stream_bytes"]          # the host plan's figure keeps its meaning
    assert np.isfinite(Y1).all() and _same_bits(Y1, Y0)
    Yref, scale = ref
    worst = float(np.max(np.abs(Y1 - Yref) / np.maximum(scale, np.finfo(float).tiny)))
    print("%s: worst |Y - Yref| / (|A| |X|) = %.3e" % (case, worst))
    np.testing.assert_allclose(Y1, Yref, rtol=1e-12, atol=1e-12 * np.abs(Yref).max())
    assert np.all(np.abs(Y1 - Yref) <= 1e-12 * scale)


def test_packed_products_on_a_shard_with_halo_slots(monkeypatch):
    """Rank 1 of 3 rehearsed in this process (preAlps_hip_loopback): the forced run plan holds halo slots, its
    interior and its halo-reading blocks are both on the list."""
    import prealps_amd
    mat = _matrix("poisson12")
    L = prealps_amd.load()
    try:
        Y1, s1, _ = _product(monkeypatch, mat, 4, 1, 9, {"PREALPS_SPMM_RUNS": "2"}, reference=False, shard=(1, 3))
        Y0, s0, _ = _product(monkeypatch, mat, 4, 0, 9, {"PREALPS_SPMM_RUNS": "2"}, reference=False, shard=(1, 3))
    finally:                                              # one process, no hooks, for the tests that follow
        L.preAlps_hip_set_world(0, 1)
        L.preAlps_hip_set_comm(prealps_amd.lib.ALLREDUCE_FN(), prealps_amd.lib.EXCHANGE_FN(), None)
    assert s1["halo_rows"] > 0 and s1["spmm_packed"] == 1 and s0["spmm_packed"] == 0 and s1["spmm_runs"] == s0["spmm_runs"] == 1
    assert np.isfinite(Y1).all() and np.any(Y1 != 0.0) and _same_bits(Y1, Y0)


def test_solver_history_and_solution_have_the_same_bits(monkeypatch):
    """Elasticity 9^3, boxes of 3^3 nodes, t = 4, Orthodir, the library's loop: the Gram kernel on the packed plan."""
    import prealps_amd as pa
    mat = _matrix("elasticity9")
    got = {}
    for pack in (1, 0):
        _env(monkeypatch, PREALPS_SPMM_PACK=pack)
        prob = _problem(*mat)
        try:
            rhs = prob.reference_rhs()
            before = prob.stat("spmm_gram_launches")
            r = prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, tol=1e-5)
            got[pack] = (r, prob.stat("spmm_gram_launches") - before, prob.stat("spmm_packed"))
        finally:
            prob.close()
    (r1, g1, p1), (r0, g0, p0) = got[1], got[0]
    print("elasticity9: %d iterations, %d launches with the Gram block" % (r1.iters, g1))
    assert p1 == 1 and p0 == 0
    assert 0 < r1.iters == r0.iters < 1000 and g1 == g0 > 0
    assert _same_bits(r1.res, r0.res) and _same_bits(r1.x, r0.x)


def _scaled(rp, ci, v):                   # S A S (test_gpu_update_values.py): every value changes, zeros stay zero
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    rows = np.repeat(np.arange(N), np.diff(rp))
    return s[rows] * v * s[ci]


def test_update_writes_through_the_pack_or_packs_anew(monkeypatch):
    rp, ci, v, P, part = _matrix("elasticity7")
    v2 = _scaled(rp, ci, v)
    v3 = v2.copy()
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    zero = np.flatnonzero((v2.view(np.uint64) == 0) & (rows != ci))
    assert len(zero) > 0
    k = zero[len(zero) // 2]                                  # one dropped entry and its mirror image become nonzero
    mirror = np.flatnonzero((rows == ci[k]) & (ci == rows[k]))[0]
    v3[k] = v3[mirror] = -1e-3
    X = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    _env(monkeypatch, PREALPS_SPMM_PACK=1)
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.block_operator(X, 4)
        assert prob.stat("spmm_packed") == 1
        at, kept = prob.stat("spmm_val_address"), prob.stat("spmm_packed_values")
        prob.update_values(v2)
        assert prob.stat("spmm_val_address") == at and prob.stat("spmm_repacks") == 0
        map_bytes = prob.stat("op_value_map_bytes")
        assert map_bytes >= 4 * prob.stat("spmm_stored_entries")
        Y2 = prob.block_operator(X, 4)
        assert prob.L.preAlps_hip_debug_move_plan(3) == 0
        assert prob.stat("spmm_val_address") != at
        Y2_moved = prob.block_operator(X, 4)
        prob.update_values(v3)
        assert prob.stat("spmm_repacks") == 1 and prob.stat("spmm_packed") == 1
        assert prob.stat("spmm_packed_values") > kept and prob.stat("op_value_map_bytes") >= map_bytes
        Y3 = prob.block_operator(X, 4)
        prob.update_values(v2)                                # the new places stay; they hold +0.0 again
        assert prob.stat("spmm_repacks") == 1
        Y2_again = prob.block_operator(X, 4)
    finally:
        prob.close()
    fresh = {}
    for name, vals in (("v2", v2), ("v3", v3)):
        for pack in (1, 0):
            _env(monkeypatch, PREALPS_SPMM_PACK=pack)
            f = _problem(rp, ci, vals, P, part)
            try:
                fresh[name, pack] = f.block_operator(X, 4)
            finally:
                f.close()
    assert _same_bits(fresh["v2", 1], fresh["v2", 0]) and _same_bits(fresh["v3", 1], fresh["v3", 0])
    assert _same_bits(Y2, fresh["v2", 1]) and _same_bits(Y2_moved, Y2) and _same_bits(Y2_again, Y2)
    assert _same_bits(Y3, fresh["v3", 1]) and not np.array_equal(Y3, Y2)


def test_the_default_packs_elasticity_and_not_poisson(monkeypatch):
    _, s, _ = _product(monkeypatch, _matrix("elasticity9"), 4, None, 3, reference=False)
    print("elasticity9: stream %.0f -> %.0f bytes" % (s["spmm_stream_bytes"], s["spmm_packed_stream_bytes"]))
    assert s["spmm_packed"] == 1 and s["spmm_runs"] == 1
    assert s["spmm_packed_stream_bytes"] < 0.9 * s["spmm_stream_bytes"]
    _, s, _ = _product(monkeypatch, _matrix("poisson12"), 4, None, 3, reference=False)
    assert s["spmm_packed"] == 0
