"""The matrix values of the SpMM in single precision (preAlps_hip_set_operator_precision(32), PREALPS_SPMM_PRECISION,
EcgProblem.set_operator_precision("single")): the packed run plan at up to 4 columns streams a fp32 copy of its packed
value array through the same masks, widens every value exactly and runs the FMAs of the fp64 kernel in its order.  So

  1. a product has the BITS of the fp64 kernel on the matrix whose values are the rounded ones;
  2. on a scaled operator it lies within the derived row-wise bound of test_gpu_spmm_blocks.py around B_v32 X, and
     outside that bound around B_v X (the storage really is fp32);
  3. plans the switch does not reach keep fp64 and the bits of a problem that never heard of it;
  4. switching back and forth inside one problem restores the bits, and the fp64 array never moves;
  5. an update of the values rounds the copy again (in place, or anew after a repack);
  6. the Gram kernel on the fp32 copy gives the histories of the plain kernel plus k_gram, as it does in fp64;
  7. a value that fp32 cannot hold is refused by name.

The matrices are those of test_gpu_spmm_pack.py."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_spmm_pack as TP

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RTOL_HIST = 1e-8            # two fp64 implementations of one iteration (test_gpu_configs.py / test_gpu_parity.py)
_SWITCHES = TP._SWITCHES + ("PREALPS_SPMM_PRECISION",)
_STATS = ("spmm_precision", "spmm_val32_bytes", "spmm_val32_address", "spmm_val_address", "spmm_packed", "spmm_runs",
          "spmm_packed_values", "spmm_stored_entries", "spmm_packed_stream_bytes", "spmm_precision_stream_bytes",
          "spmm_stream_bytes", "spmm_repacks", "halo_rows", "spmm_round_kernel_s")
PACK_SLACK = 64             # spmm_pack.h


def _env(monkeypatch, **env):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _same_bits(a, b):
    return TP._same_bits(a, b)


def _round32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _stats(prob):
    return {k: prob.stat(k) for k in _STATS}


def _open(mat, scale, precision=None, **kw):
    import prealps_amd
    rp, ci, v, P, part = mat
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=scale, device=0, **kw)
    if precision is not None:
        prob.set_operator_precision(precision)
    return prob


def _products(mat, t, scale, precision, seed, repeats=1, **kw):
    """`repeats` products Y = A X of a fresh operator at the given storage, and the statistics of the plan that ran."""
    prob = _open(mat, scale, precision, **kw)
    try:
        X = np.random.default_rng(seed).standard_normal((prob.m, t))
        Ys = [prob.block_operator(X, t) for _ in range(repeats)]
        return Ys, _stats(prob)
    finally:
        prob.close()


def _packed_elements(s):
    """Elements of the packed array: one zero per step (192 stored values), the kept values, the slack."""
    assert s["spmm_stored_entries"] % 192 == 0
    return s["spmm_stored_entries"] / 192 + s["spmm_packed_values"] + PACK_SLACK


# ---- 1. bits ----------------------------------------------------------------------------------------------------
_BITS = {
    "elasticity7-t1": ("elasticity7", 1, {}, {}),
    "elasticity7-t2": ("elasticity7", 2, {}, {}),
    "elasticity7-t4": ("elasticity7", 4, {}, {}),
    "ragged-blocks-of-four-t4": ("ragged", 4, {"PREALPS_SPMM_RUNS": "2"}, {}),
    "poisson12-shard-1-of-3-t4": ("poisson12", 4, {"PREALPS_SPMM_RUNS": "2"}, {"shard": (1, 3)}),
}


@pytest.mark.parametrize("case", list(_BITS))
def test_single_storage_has_the_bits_of_the_fp64_kernel_on_the_rounded_matrix(case, monkeypatch):
    import prealps_amd
    kind, t, env, kw = _BITS[case]
    rp, ci, v, P, part = TP._matrix(kind)
    v32 = _round32(v)
    # rounding keeps the set of stored +0.0 (what the pack drops) and of zeros altogether: nothing underflows
    assert np.array_equal(v.view(np.uint64) == 0, v32.view(np.uint64) == 0) and np.array_equal(v == 0.0, v32 == 0.0)
    L = prealps_amd.load()
    try:
        _env(monkeypatch, **env)
        YA, sA = _products((rp, ci, v, P, part), t, False, "single", 21, repeats=3, **kw)
        _env(monkeypatch, PREALPS_SPMM_PACK=1, **env)
        YB, sB = _products((rp, ci, v32, P, part), t, False, "double", 21, repeats=3, **kw)
    finally:
        if kw:                                            # one process, no hooks, for the tests that follow
            L.preAlps_hip_set_world(0, 1)
            L.preAlps_hip_set_comm(prealps_amd.lib.ALLREDUCE_FN(), prealps_amd.lib.EXCHANGE_FN(), None)
    print("%s: %d packed elements, one product streams %.0f (fp64) -> %.0f (fp32) bytes, rounding kernel %.1f us" % (
        case, _packed_elements(sA), sA["spmm_packed_stream_bytes"], sA["spmm_precision_stream_bytes"],
        1e6 * sA["spmm_round_kernel_s"]))
    assert sA["spmm_precision"] == 32 and sB["spmm_precision"] == 64
    assert sA["spmm_packed"] == sB["spmm_packed"] == 1 and sA["spmm_runs"] == sB["spmm_runs"] == 1
    assert sA["spmm_val32_bytes"] == 4 * _packed_elements(sA) and sA["spmm_val32_address"] != 0
    assert sB["spmm_val32_bytes"] == 0 and sB["spmm_val32_address"] == 0
    assert sA["spmm_packed_values"] == sB["spmm_packed_values"]
    assert sA["spmm_precision_stream_bytes"] == sA["spmm_packed_stream_bytes"] - 4 * (_packed_elements(sA) - PACK_SLACK)
    assert sB["spmm_precision_stream_bytes"] == sB["spmm_packed_stream_bytes"]
    if kw:
        assert sA["halo_rows"] > 0
    assert np.isfinite(YA[0]).all() and np.any(YA[0] != 0.0)
    assert _same_bits(YA[0], YB[0])
    assert all(_same_bits(y, YA[0]) for y in YA[1:]) and all(_same_bits(y, YB[0]) for y in YB[1:])


# ---- 2. the scaled operator, by the derived bound --------------------------------------------------------------
def test_scaled_product_lies_within_the_bound_of_the_rounded_matrix_and_outside_that_of_the_given_one(monkeypatch):
    _env(monkeypatch)
    prob = _open(TP._matrix("elasticity12"), True, "single")
    try:
        X = np.random.default_rng(33).standard_normal((prob.m, 4))
        Y = prob.block_operator(X, 4)
        assert prob.stat("spmm_precision") == 32
        rp, ci, v = prob.local_csr()
    finally:
        prob.close()
    shape = (len(rp) - 1, len(rp) - 1)
    terms = (np.diff(rp) + 2).astype(np.float64)[:, None]
    Xl = X.astype(np.longdouble)
    worst = {}
    for name, vals in (("v32", _round32(v)), ("v", v)):
        Yref = sp.csr_matrix((vals.astype(np.longdouble), ci, rp), shape=shape) @ Xl
        limit = terms * U * (sp.csr_matrix((np.abs(vals), ci, rp), shape=shape) @ np.abs(X))
        assert Yref.dtype == np.longdouble and np.all(limit > 0)
        worst[name] = np.abs(Y - Yref).astype(np.float64) / limit
    print("elasticity12 scaled, single: worst |Y - B X| / limit = %.3f against B_v32, %.3e against B_v" % (
        worst["v32"].max(), worst["v"].max()))
    assert np.isfinite(Y).all()
    assert np.all(worst["v32"] <= 1.0)
    assert np.any(worst["v"] > 1.0)


# ---- 3. where the switch does not reach -------------------------------------------------------------------------
@pytest.mark.parametrize("kind,t", [("elasticity12", 8), ("poisson12", 4)], ids=["8-columns", "window-plan"])
def test_plans_out_of_reach_keep_fp64_and_their_bits(kind, t, monkeypatch):
    _env(monkeypatch)
    mat = TP._matrix(kind)
    (Y1,), s1 = _products(mat, t, True, "single", 5)
    (Y0,), s0 = _products(mat, t, True, None, 5)                  # a problem that never heard of the switch
    assert s1["spmm_precision"] == 64 and s1["spmm_val32_bytes"] == 0 and s0["spmm_precision"] == 64
    assert s1["spmm_packed"] == s0["spmm_packed"] and s1["spmm_runs"] == s0["spmm_runs"]
    assert s1["spmm_precision_stream_bytes"] == s0["spmm_precision_stream_bytes"] > 0
    assert np.isfinite(Y1).all() and _same_bits(Y1, Y0)


def test_pack_0_wins_and_the_variable_selects_like_the_call(monkeypatch):
    mat = TP._matrix("elasticity7")
    _env(monkeypatch, PREALPS_SPMM_PACK=0)
    (Y1,), s1 = _products(mat, 4, True, "single", 6)
    assert s1["spmm_precision"] == 64 and s1["spmm_packed"] == 0 and s1["spmm_runs"] == 1
    _env(monkeypatch, PREALPS_SPMM_PRECISION="single")
    (Y2,), s2 = _products(mat, 4, True, None, 6)
    _env(monkeypatch)
    (Y3,), s3 = _products(mat, 4, True, "single", 6)
    (Y0,), s0 = _products(mat, 4, True, None, 6)
    assert s2["spmm_precision"] == s3["spmm_precision"] == 32 and s0["spmm_precision"] == 64
    assert _same_bits(Y2, Y3) and _same_bits(Y1, Y0) and not np.array_equal(Y2, Y0)


# ---- 4. switching inside one problem ----------------------------------------------------------------------------
def test_switching_restores_the_bits_and_never_moves_the_fp64_values(monkeypatch):
    _env(monkeypatch)
    prob = _open(TP._matrix("elasticity12"), True)
    try:
        X = np.random.default_rng(8).standard_normal((prob.m, 4))
        Y0 = prob.block_operator(X, 4)
        s0 = _stats(prob)
        prob.set_operator_precision("single")
        s1 = _stats(prob)                                         # at once: the copy is formed inside the call
        Y1 = prob.block_operator(X, 4)
        prob.set_operator_precision("double")
        s2 = _stats(prob)
        Y2 = prob.block_operator(X, 4)
        prob.set_operator_precision("single")
        Y3 = prob.block_operator(X, 4)
    finally:
        prob.close()
    assert s0["spmm_precision"] == 64 and s0["spmm_val32_bytes"] == 0 and s0["spmm_packed"] == 1
    assert s1["spmm_precision"] == 32 and s1["spmm_val32_bytes"] == 4 * _packed_elements(s1)
    assert s2["spmm_precision"] == 64 and s2["spmm_val32_bytes"] == 0 and s2["spmm_val32_address"] == 0
    assert s0["spmm_val_address"] == s1["spmm_val_address"] == s2["spmm_val_address"] != 0
    assert _same_bits(Y2, Y0) and _same_bits(Y3, Y1) and not np.array_equal(Y1, Y0)


# ---- 5. new values ----------------------------------------------------------------------------------------------
def test_an_update_of_the_values_rounds_the_copy_again(monkeypatch):
    rp, ci, v, P, part = TP._matrix("elasticity7")
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    # (not S A S of test_gpu_spmm_pack.py: where the diagonal is the largest entry of its row the scaling of the
    # build undoes a diagonal S but for the last bits, which the rounding to fp32 then removes -- the same bits)
    w = np.random.default_rng(20261020).random(len(rp) - 1)
    v2 = v * (1.0 + 0.1 * w[rows] * w[ci])                    # symmetric, every value changes, zeros stay zero
    v3 = v2.copy()
    zero = np.flatnonzero((v2.view(np.uint64) == 0) & (rows != ci))
    assert len(zero) > 0
    k = zero[len(zero) // 2]                                  # one dropped entry and its mirror image become nonzero
    mirror = np.flatnonzero((rows == ci[k]) & (ci == rows[k]))[0]
    v3[k] = v3[mirror] = -1e-3
    _env(monkeypatch)
    prob = _open((rp, ci, v, P, part), True, "single")
    try:
        X = np.random.default_rng(4).standard_normal((prob.m, 4))
        Y1 = prob.block_operator(X, 4)
        s1 = _stats(prob)
        prob.update_values(v2)                                    # the same zero set: written through, rounded in place
        s2 = _stats(prob)
        Y2 = prob.block_operator(X, 4)
        prob.update_values(v3)                                    # a dropped +0.0 becomes nonzero: packed anew
        s3 = _stats(prob)
        Y3 = prob.block_operator(X, 4)
    finally:
        prob.close()
    assert s1["spmm_precision"] == s2["spmm_precision"] == s3["spmm_precision"] == 32
    assert s2["spmm_repacks"] == 0 and s2["spmm_val32_address"] == s1["spmm_val32_address"] != 0
    assert s2["spmm_val_address"] == s1["spmm_val_address"]
    assert s3["spmm_repacks"] == 1 and s3["spmm_packed_values"] > s2["spmm_packed_values"]
    assert s3["spmm_val32_bytes"] == 4 * _packed_elements(s3) > s2["spmm_val32_bytes"]
    (F2,), _ = _products((rp, ci, v2, P, part), 4, True, "single", 4)
    (F3,), _ = _products((rp, ci, v3, P, part), 4, True, "single", 4)
    (D2,), _ = _products((rp, ci, v2, P, part), 4, True, "double", 4)
    assert _same_bits(Y2, F2) and _same_bits(Y3, F3)
    assert not np.array_equal(Y2, Y1) and not np.array_equal(Y3, Y2) and not np.array_equal(F2, D2)


# ---- 6. the Gram kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["single", "double"])
def test_gram_kernel_follows_the_plain_kernel(precision, monkeypatch):
    """Elasticity 9^3, boxes of 3^3 nodes, t = 4, Orthodir, the library's loop: k_spmm_runs_gram_pack against
    k_spmm_runs_pack followed by k_gram, on the same storage."""
    import prealps_amd as pa
    mat = TP._matrix("elasticity9")
    got = {}
    for gram in (None, 0):
        _env(monkeypatch, **({} if gram is None else {"PREALPS_SPMM_GRAM": gram}))
        prob = _open(mat, True, precision)
        try:
            rhs = prob.reference_rhs()
            before = prob.stat("spmm_gram_launches")
            r = prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, tol=1e-5)
            got[gram] = (r, prob.stat("spmm_gram_launches") - before, prob.stat("spmm_precision"))
        finally:
            prob.close()
    (r1, g1, p1), (r0, g0, p0) = got[None], got[0]
    print("elasticity9 %s: %d iterations, %d launches with the Gram block, histories differ by %.2e relative" % (
        precision, r1.iters, g1, np.max(np.abs(r1.res - r0.res) / r0.res) if r1.iters == r0.iters else np.nan))
    assert p1 == p0 == (32 if precision == "single" else 64)
    assert 0 < r1.iters == r0.iters < 1000
    assert g1 >= r1.iters and g0 == 0
    np.testing.assert_allclose(r1.res, r0.res, rtol=RTOL_HIST)


# ---- 7. a value that fp32 cannot hold ----------------------------------------------------------------------------
def test_a_value_beyond_fp32_is_refused_by_name(monkeypatch):
    import prealps_amd as pa
    rp, ci, v, P, part = TP._matrix("elasticity7")
    v = v.copy()
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    diag = np.flatnonzero(rows == ci)
    v[diag[len(diag) // 2]] = 1e39                            # finite in fp64, +Inf in fp32; the matrix stays SPD
    _env(monkeypatch)
    prob = _open((rp, ci, v, P, part), False)
    try:
        X = np.random.default_rng(2).standard_normal((prob.m, 4))
        Y0 = prob.block_operator(X, 4)
        with pytest.raises(pa.PreAlpsError, match="single precision") as e:
            prob.set_operator_precision("single")             # an existing plan: the call itself fails
        named = re.search(r"one of them: ([^)]+)\)", str(e.value))
        assert named and float(named.group(1)) == 1e39
        assert prob.stat("spmm_precision") == 64 and prob.stat("spmm_val32_bytes") == 0
        prob.set_operator_precision("double")
        Y1 = prob.block_operator(X, 4)
    finally:
        prob.close()
    assert np.isfinite(Y0).all() and _same_bits(Y1, Y0)
    prob = _open((rp, ci, v, P, part), False, "single")       # no plan yet: the product that cuts it fails
    try:
        with pytest.raises(pa.PreAlpsError, match="single precision"):
            prob.block_operator(X, 4)
        prob.set_operator_precision("double")
        Y2 = prob.block_operator(X, 4)
    finally:
        prob.close()
    assert _same_bits(Y2, Y0)
    # new values that fp32 cannot hold: the update is refused by name (the fp64 values are in place by then), products
    # fail while single stays in force, and double gives the fresh double problem's bits again -- in place and anew
    v0 = v.copy()
    v0[diag[len(diag) // 2]] = TP._matrix("elasticity7")[2][diag[len(diag) // 2]]
    zero = np.flatnonzero((v0.view(np.uint64) == 0) & (rows != ci))
    k = zero[len(zero) // 2]
    mirror = np.flatnonzero((rows == ci[k]) & (ci == rows[k]))[0]
    v_new = v.copy()
    v_new[k] = v_new[mirror] = -1e-3                          # with the 1e39: a dropped +0.0 becomes nonzero, a repack
    for name, vals, repacks in (("write-through", v, 0), ("repack", v_new, 1)):
        prob = _open((rp, ci, v0, P, part), False, "single")
        try:
            prob.block_operator(X, 4)
            assert prob.stat("spmm_precision") == 32
            with pytest.raises(pa.PreAlpsError, match="single precision"):
                prob.update_values(vals)
            assert prob.stat("spmm_repacks") == repacks and prob.stat("spmm_val32_bytes") == 0
            with pytest.raises(pa.PreAlpsError, match="single precision"):
                prob.block_operator(X, 4)                     # single is still in force: no quiet fp64 product
            prob.set_operator_precision("double")
            Y3 = prob.block_operator(X, 4)
            assert prob.stat("spmm_precision") == 64 and prob.stat("spmm_val32_bytes") == 0
            prob.update_values(v0)                            # values that fit again: double stays double
            Y4 = prob.block_operator(X, 4)
            assert prob.stat("spmm_precision") == 64 and prob.stat("spmm_val32_bytes") == 0
        finally:
            prob.close()
        (F3,), sF = _products((rp, ci, vals, P, part), 4, False, "double", 2)
        (F4,), _ = _products((rp, ci, v0, P, part), 4, False, "double", 2)
        assert sF["spmm_precision"] == 64 and _same_bits(Y3, F3) and _same_bits(Y4, F4), name
