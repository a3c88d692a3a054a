"""preAlps_OperatorUpdateValues on the device: after new values for the same pattern, every product -- through the
window, the staged and the run plan, at 4, 8 and 16 columns, on a moved plan and on a shard with halo slots -- has
the bits of a fresh build from those values, the plan's device arrays keep their addresses, and a solve on the
updated operator is the fresh problem's solve (factor rebuilt) or converges with the lagged factor (factor kept)."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

_PLAN_STATS = ("spmm_runs", "spmm_staged", "spmm_blocks", "spmm_slices", "spmm_stored_entries",
               "spmm_stream_bytes", "spmm_stage_rows", "spmm_interior_blocks")

# the (problem, switches) cases of test_gpu_parity.py::test_spmm_plan_is_rebuilt_alike_when_the_stride_changes, and the
# plan (staged, runs) each must reach at every stride (None: the builder decides, 4 columns take the run plan)
_CASES = {
    "poisson-window": ("poisson", {"PREALPS_SPMM_STAGED": "0"}, (0.0, 0.0)),
    "poisson-staged": ("poisson", {"PREALPS_SPMM_STAGED": "1", "PREALPS_SPMM_RUNS": "0"}, (1.0, 0.0)),
    "elasticity-default": ("elasticity_cut", {}, None),
    "random-forced-runs": ("random", {"PREALPS_SPMM_RUNS": "2"}, (1.0, 1.0)),
}


def _random_spd(n, density, seed):
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=rng, format="csr")
    A = M + M.T
    A = A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def _new_values(rp, ci, v):
    """v2 = S A S, S = diag(1 + 0.3 (2u - 1)): the pattern stays, the matrix stays SPD, every value and the scaling
    vector change."""
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    rows = np.repeat(np.arange(N), np.diff(rp))
    return s[rows] * v * s[ci]


def _matrix(kind):
    """rowptr, colind, val, val2, number of parts, partition vector."""
    from oracle import oracle as O
    from prealps_amd import gen
    if kind == "random":
        A, P = _random_spd(1500, 0.004, 11), 7
    elif kind in ("poisson", "poisson-shard"):
        A, P = O.poisson3d(12), 5
    elif kind == "elasticity_cut":
        rp, ci, v = gen.elasticity3d_csr(7)
        A, P = sp.csr_matrix((v, ci, rp), shape=(3 * 343, 3 * 343)), 8
    elif kind == "poisson10":
        rp, ci, v = gen.poisson3d_csr(10)
        part, P = gen.box_partition(10, (5, 5, 5))
        return rp, ci, v, _new_values(rp, ci, v), P, part
    elif kind == "elasticity12":
        nn = (12, 10, 10)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, P = gen.box_partition_nodes(nn, (2, 2, 2))
        return rp, ci, v, _new_values(rp, ci, v), P, part
    rp, ci, v = O.as_csr(A)
    return rp, ci, v, _new_values(rp, ci, v), P, O.contiguous_partition(A.shape[0], P)


def _switches(monkeypatch, env):
    for k in ("PREALPS_SPMM_STAGED", "PREALPS_SPMM_RUNS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _problem(rp, ci, v, P, part, **kw):
    import prealps_amd
    return prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fresh_product(rp, ci, v2, P, part, X, t, **kw):
    fresh = _problem(rp, ci, v2, P, part, **kw)
    try:
        Y = fresh.block_operator(X, t)
        return Y, {k: fresh.stat(k) for k in _PLAN_STATS}
    finally:
        fresh.close()


@pytest.mark.parametrize("t", [4, 8, 16])
@pytest.mark.parametrize("case", list(_CASES))
def test_updated_products_have_the_bits_of_a_fresh_build(case, t, monkeypatch):
    kind, env, want_plan = _CASES[case]
    _switches(monkeypatch, env)
    rp, ci, v, v2, P, part = _matrix(kind)
    X = np.random.default_rng(t).standard_normal((len(rp) - 1, t))
    prob = _problem(rp, ci, v, P, part)
    try:
        Y0 = prob.block_operator(X, t)                   # the plan exists
        before = {k: prob.stat(k) for k in _PLAN_STATS}
        val_at, slot_at = prob.stat("spmm_val_address"), prob.stat("spmm_slot_address")
        assert prob.stat("op_value_map_builds") == 0 and prob.stat("op_value_map_bytes") == 0
        prob.update_values(v2)
        assert prob.stat("spmm_val_address") == val_at and prob.stat("spmm_slot_address") == slot_at
        assert {k: prob.stat(k) for k in _PLAN_STATS} == before
        assert prob.stat("op_values_epoch") == 1 and prob.stat("op_value_map_builds") == 1
        assert prob.stat("op_value_map_bytes") >= 4 * (before["spmm_stored_entries"])
        Yu = prob.block_operator(X, t)
    finally:
        prob.close()
    Yf, fresh_stats = _fresh_product(rp, ci, v2, P, part, X, t)
    plan = (before["spmm_staged"], before["spmm_runs"])
    print("%s t=%d: plan (staged, runs) = %s, %d stored entries" % (case, t, plan, before["spmm_stored_entries"]))
    assert _same_bits(Yu, Yf)
    assert not np.array_equal(Yu, Y0)
    assert fresh_stats == before                          # the pattern decides the plan, not the values
    if want_plan is not None:
        assert plan == want_plan                          # window, staged and run plans are all among the cases
    elif t == 4:
        assert plan == (1.0, 1.0)


@pytest.mark.parametrize("case", ["poisson-window", "elasticity-default"])
def test_update_before_any_product_and_at_another_stride(case, monkeypatch):
    kind, env, _ = _CASES[case]
    _switches(monkeypatch, env)
    rp, ci, v, v2, P, part = _matrix(kind)
    X4 = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    X8 = np.random.default_rng(8).standard_normal((len(rp) - 1, 8))
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.update_values(v2)                            # no plan yet: the host panel alone
        assert prob.stat("op_value_map_builds") == 0
        first = prob.block_operator(X4, 4)                # the plan is cut from the new values
        prob.update_values(v)                             # a plan of stride 4 is on the device: map and kernel
        assert prob.stat("op_value_map_builds") == 1 and prob.stat("op_value_map_bytes") > 0
        prob.update_values(v2)
        assert prob.stat("op_value_map_builds") == 1
        wide = prob.block_operator(X8, 8)                 # another stride: a new plan from the host panel, no map
        assert prob.stat("op_value_map_bytes") == 0
        prob.update_values(v)
        prob.update_values(v2)
        assert prob.stat("op_value_map_builds") == 2 and prob.stat("op_values_epoch") == 5
        wide_again = prob.block_operator(X8, 8)
    finally:
        prob.close()
    assert _same_bits(first, _fresh_product(rp, ci, v2, P, part, X4, 4)[0])
    want8 = _fresh_product(rp, ci, v2, P, part, X8, 8)[0]
    assert _same_bits(wide, want8) and _same_bits(wide_again, want8)


@pytest.mark.parametrize("case", ["poisson-window", "poisson-staged", "random-forced-runs"])
def test_two_updates_give_the_first_product_again(case, monkeypatch):
    kind, env, _ = _CASES[case]
    _switches(monkeypatch, env)
    rp, ci, v, v2, P, part = _matrix(kind)
    X = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    prob = _problem(rp, ci, v, P, part)
    try:
        Y0 = prob.block_operator(X, 4)
        prob.update_values(v2)
        Y1 = prob.block_operator(X, 4)
        prob.update_values(v)
        Y2 = prob.block_operator(X, 4)
        assert prob.stat("op_value_map_builds") == 1 and prob.stat("op_values_epoch") == 2
    finally:
        prob.close()
    assert _same_bits(Y2, Y0) and not np.array_equal(Y1, Y0)


def test_update_writes_to_a_moved_run_plan(monkeypatch):
    _switches(monkeypatch, {})
    rp, ci, v, v2, P, part = _matrix("elasticity_cut")
    X = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    prob = _problem(rp, ci, v, P, part)
    try:
        prob.block_operator(X, 4)
        assert prob.stat("spmm_runs") == 1.0
        val_at = prob.stat("spmm_val_address")
        assert prob.L.preAlps_hip_debug_move_plan(3) == 0
        moved_to = prob.stat("spmm_val_address")
        assert moved_to != val_at
        prob.update_values(v2)
        assert prob.stat("spmm_val_address") == moved_to
        Yu = prob.block_operator(X, 4)
    finally:
        prob.close()
    assert _same_bits(Yu, _fresh_product(rp, ci, v2, P, part, X, 4)[0])


def test_update_on_a_shard_with_halo_slots(monkeypatch):
    """Rank 1 of 3 rehearsed in this process (preAlps_hip_loopback): the forced run plan holds halo slots."""
    import prealps_amd
    _switches(monkeypatch, {"PREALPS_SPMM_RUNS": "2"})
    rp, ci, v, v2, P, part = _matrix("poisson-shard")
    L = prealps_amd.load()
    try:
        prob = _problem(rp, ci, v, P, part, shard=(1, 3))
        try:
            assert prob.stat("halo_rows") > 0 and prob.m < len(rp) - 1
            X = np.random.default_rng(4).standard_normal((prob.m, 4))
            Y0 = prob.block_operator(X, 4)
            assert prob.stat("spmm_runs") == 1.0
            val_at = prob.stat("spmm_val_address")
            prob.update_values(v2)
            assert prob.stat("spmm_val_address") == val_at
            Yu = prob.block_operator(X, 4)
        finally:
            prob.close()
        Yf = _fresh_product(rp, ci, v2, P, part, X, 4, shard=(1, 3))[0]
    finally:                                              # one process, no hooks, for the tests that follow
        L.preAlps_hip_set_world(0, 1)
        L.preAlps_hip_set_comm(prealps_amd.lib.ALLREDUCE_FN(), prealps_amd.lib.EXCHANGE_FN(), None)
    assert _same_bits(Yu, Yf) and not np.array_equal(Yu, Y0)


@pytest.mark.parametrize("kind", ["poisson10", "elasticity12"])
def test_solve_after_an_update_with_the_factor_rebuilt(kind, monkeypatch):
    import prealps_amd as pa
    _switches(monkeypatch, {})
    rp, ci, v, v2, P, part = _matrix(kind)
    t = 4
    prob = _problem(rp, ci, v, P, part)
    try:
        rhs = prob.reference_rhs()
        old = prob.solve(rhs, t, ortho_alg=pa.ORTHODIR, tol=1e-5)     # plan and factor of the old values are in use
        prob.update_values(v2, precond="rebuild")
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


@pytest.mark.parametrize("kind", ["poisson10", "elasticity12"])
def test_solve_after_an_update_with_the_lagged_factor(kind, monkeypatch):
    """The factor of the old values stays: a lagged, still SPD preconditioner.  The solve converges, and its x has
    the true residual ||b - A2 x|| <= 2 sqrt(t) tol ||b|| on the updated panel (the bound and margin of
    test_gpu_nd_precision.py::test_ecg_with_single_precision_factor: the stopping test sees the t columns of R, whose
    sum is the residual)."""
    import prealps_amd as pa
    _switches(monkeypatch, {})
    rp, ci, v, v2, P, part = _matrix(kind)
    t, tol, max_iter = 4, 1e-5, 1000
    prob = _problem(rp, ci, v, P, part)
    try:
        rhs = prob.reference_rhs()
        prob.solve(rhs, t, ortho_alg=pa.ORTHODIR, tol=tol, max_iter=max_iter)
        prob.update_values(v2, precond="keep")
        assert prob.stat("bj_values_epoch") < prob.stat("op_values_epoch")
        lagged = prob.solve(rhs, t, ortho_alg=pa.ORTHODIR, tol=tol, max_iter=max_iter)
        lrp, lci, lv = prob.local_csr()
        prob.update_values(v2, precond="rebuild")
        assert prob.stat("bj_values_epoch") == prob.stat("op_values_epoch") == 2
        rebuilt = prob.solve(rhs, t, ortho_alg=pa.ORTHODIR, tol=tol, max_iter=max_iter)
    finally:
        prob.close()
    A2 = sp.csr_matrix((lv, lci, lrp), shape=(len(rhs), len(rhs)))
    true_res = float(np.linalg.norm(rhs - A2 @ lagged.x) / np.linalg.norm(rhs))
    print("%s: %d iterations with the lagged factor, %d with the rebuilt one, true residual %.3e"
          % (kind, lagged.iters, rebuilt.iters, true_res))
    assert lagged.iters < max_iter and lagged.final_res <= tol * lagged.normb
    assert true_res <= 2.0 * np.sqrt(t) * tol
