"""preAlps_ECGSolveSystemRefined / EcgProblem.solve_system(..., refine=True): a system solve in passes, every pass after
the first started from the x before it with a start residual formed on the fp64 values of the matrix -- what makes the
single-precision storage of the operator (set_operator_precision("single")) safe to solve with.

The problem is E of test_gpu_system_solve.py: elasticity on 12 x 10 x 10 nodes, boxes of 2 x 2 x 2 nodes, scaled;
tol = 1e-5, stop="original", the right-hand sides of that file (default_rng(20260407).standard_normal), k = 1 and k = 2
systems at t = 4.

8.  On the host, the exact (splu) solve of the rounded scaled matrix leaves ||b - A x|| / ||b|| above tol for every
    system used (measured on the host: 1.5e-4 .. 6.0e-4 for the first four right-hand sides): the input does need
    the repair.
9.  single, refine=False: xa, with the true ratio ra.
10. single, refine=True: every true ratio <= 1.01 tol (that file's margin), converged, pass_res[0] = ||b_j||,
    pass_res[1] = ra ||b_j|| within twice the cancellation bound of forming b - A xa in fp64 -- the start residual of
    pass 1 comes from the fp64 values of the original matrix, not from the rounded ones --, at least two passes where
    ra > tol, and the counts and histories add up.
11. double, refine=True meets the same true-ratio test.
12. max_passes = 1 reports "out of passes" and returns xa bit for bit; max_passes = 0 and 17 are refused by name.
13. A second pass that the iteration budget cuts after five iterations -- a restarted iteration has not recovered by
    then -- reports "out of iterations" and hands back an iterate that is no worse than xa."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import test_gpu_system_solve as TS

pytestmark = pytest.mark.gpu

TOL = 1e-5
U53 = 2.0 ** -53
CASES = [(1, 4), (2, 4)]            # (systems, enlarging factor)
_state = {}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def pb():
    """The open problem E and what the host knows of it; closed (and the storage switch put back) at the end.
    8.  Before the input is used by any test: exact solves with the rounded scaled matrix, carried back to the caller's
    space, miss the tolerance for every system used."""
    import prealps_amd as pa
    rp, ci, v, part, P = TS._matrix("E")
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    try:
        prob.create_block_jacobi()
        A0 = sp.csr_matrix((v, ci, rp), shape=(prob.N, prob.N))
        d = TS._describe(prob, A0)
        A = d["A"].copy()
        A.data = A.data.astype(np.float32).astype(np.float64)
        assert np.array_equal(A.data == 0.0, d["A"].data == 0.0) and abs(A - A.T).max() == 0.0
        B = d["B"][:, :2]
        X = TS._x_from_lib(d, spl.splu(sp.csc_matrix(A)).solve(TS._b_to_lib(d, B)))
        d["precondition"] = TS._true_ratio(d, B, X)
        print("exact solve with the rounded matrix: true ratios", d["precondition"])
        assert np.all(d["precondition"] > TOL)
        yield d
    finally:
        prob.close()


def _rhs(pb, k):
    B = pb["B"][:, :k]
    return B[:, 0].copy() if k == 1 else np.ascontiguousarray(B)


def _cols(x):
    return x[:, None] if x.ndim == 1 else x


def _solve(pb, precision, k, t, **kw):
    """One solve_system at the given storage, cached: every test reads the same result."""
    key = (precision, k, t, tuple(sorted(kw.items())))
    if key not in _state:
        prob = pb["prob"]
        prob.set_operator_precision(precision)
        try:
            r = prob.solve_system(_rhs(pb, k), t, stop="original", tol=TOL, **kw)
            r.spmm_precision = prob.stat("spmm_precision")
        finally:
            prob.set_operator_precision("double")
        _state[key] = r
    return _state[key]


def test_the_rounded_matrix_alone_misses_the_tolerance(pb):
    """8.  The fixture asserts it before any test uses the input; here its figures, within what was measured on the
    host when the test was written (1.5e-4 .. 6.0e-4)."""
    ratio = pb["precondition"]
    assert ratio.shape == (2,) and np.all(ratio > TOL) and np.all(ratio < 1e-2)


@pytest.mark.parametrize("k,t", CASES)
def test_refined_single_solve_meets_the_callers_tolerance(pb, k, t):
    """9. and 10."""
    B = _cols(_rhs(pb, k))
    plain = _solve(pb, "single", k, t)
    xa = _cols(plain.x)
    ra = TS._true_ratio(pb, B, xa)
    got = _solve(pb, "single", k, t, refine=True)
    x = _cols(got.x)
    ratio = TS._true_ratio(pb, B, x)
    nb = np.linalg.norm(B, axis=0)
    print("k=%d t=%d single: plain %d iterations, true ratios %s; refined %d passes %s iterations, true ratios %s, %s" % (
        k, t, plain.iters, ra, got.passes, got.pass_iters, ratio, got.refine_status))
    print("pass_res / ||b||:", got.pass_res / nb)
    assert plain.spmm_precision == got.spmm_precision == 32
    assert plain.passes is None and plain.refine_status is None
    assert np.all(ratio <= 1.01 * TOL)
    assert got.refine_status == "converged"
    assert got.pass_res.shape == (got.passes + 1, k) and got.pass_iters.shape == (got.passes,)
    np.testing.assert_allclose(got.pass_res[0], nb, rtol=1e-12)
    # the start residual of pass 1 is b - A xa with the fp64 values of the caller's matrix: what forming it in fp64
    # can lose is (n_max + 2) 2^-53 || |A| |xa| + |b| ||, relative to the norm of the residual itself
    cancel = (pb["n_max"] + 2) * U53 * np.linalg.norm(pb["absA0"] @ np.abs(xa) + np.abs(B), axis=0) / np.linalg.norm(
        B - pb["A0"] @ xa, axis=0)
    print("pass_res[1] against ra ||b||: relative difference %s, allowed %s" % (
        np.abs(got.pass_res[1] - ra * nb) / (ra * nb), 2 * cancel))
    assert np.all(np.abs(got.pass_res[1] - ra * nb) <= 2 * cancel * ra * nb)
    if np.any(ra > TOL):
        assert got.passes >= 2
    assert np.all(got.pass_res[got.passes] <= TOL * nb * (1 + 1e-12))
    assert int(got.pass_iters.sum()) == got.iters <= 1000
    assert got.pass_iters[0] == plain.iters and np.all(got.pass_iters[:got.passes] > 0)
    assert len(got.res) == len(got.bs) == got.iters and got.sys_hist.shape == (got.iters, k)
    assert _same_bits(got.res[:plain.iters], plain.res) and _same_bits(got.sys_hist[:plain.iters], plain.sys_hist)


@pytest.mark.parametrize("k,t", CASES)
def test_refined_double_solve_meets_the_callers_tolerance(pb, k, t):
    """11.  At fp64 the chain is a restart with the residual replaced."""
    B = _cols(_rhs(pb, k))
    got = _solve(pb, "double", k, t, refine=True)
    ratio = TS._true_ratio(pb, B, _cols(got.x))
    print("k=%d t=%d double: %d passes %s iterations, true ratios %s, %s" % (k, t, got.passes, got.pass_iters, ratio,
                                                                           got.refine_status))
    assert got.spmm_precision == 64
    assert np.all(ratio <= 1.01 * TOL) and got.refine_status == "converged"
    assert int(got.pass_iters.sum()) == got.iters == len(got.res)


def test_one_pass_is_the_plain_solve_and_the_pass_count_is_checked(pb):
    """12."""
    import prealps_amd as pa
    k, t = 1, 4
    plain = _solve(pb, "single", k, t)
    one = _solve(pb, "single", k, t, refine=True, max_passes=1)
    B = _cols(_rhs(pb, k))
    ra = TS._true_ratio(pb, B, _cols(plain.x))
    assert ra[0] > TOL                                   # (else one pass would have converged)
    assert one.refine_status == "out of passes" and one.passes == 1
    assert _same_bits(one.x, plain.x) and one.iters == plain.iters and _same_bits(one.res, plain.res)
    assert one.pass_res.shape == (2, 1) and one.pass_res[1, 0] > TOL * np.linalg.norm(B)
    prob = pb["prob"]
    for bad in (0, 17):
        with pytest.raises(pa.PreAlpsError, match="max_passes = %d" % bad) as e:
            prob.solve_system(_rhs(pb, k), t, stop="original", tol=TOL, refine=True, max_passes=bad)
        assert "preAlps_ECGSolveSystemRefined" in str(e.value)
    again = prob.solve_system(_rhs(pb, k), t, stop="original", tol=TOL)      # usable as before, fp64 again
    assert prob.stat("spmm_precision") == 64 and np.all(TS._true_ratio(pb, B, _cols(again.x)) <= 1.01 * TOL)


@pytest.mark.parametrize("extra", [1, 5])
def test_a_pass_cut_short_by_the_budget_never_hands_back_a_worse_iterate(pb, extra):
    """13.  Whichever iterate comes back, sys_res_original is ITS residual norm, within twice the cancellation bound of
    item 10."""
    k, t = 1, 4
    B = _cols(_rhs(pb, k))
    plain = _solve(pb, "single", k, t)
    ra = TS._true_ratio(pb, B, _cols(plain.x))
    got = _solve(pb, "single", k, t, refine=True, max_iter=plain.iters + extra)
    x = _cols(got.x)
    ratio = TS._true_ratio(pb, B, x)
    nb = np.linalg.norm(B, axis=0)
    print("budget %d: passes %s, %s, start ratios %s, true ratio %s (plain %s)" % (
        plain.iters + extra, got.pass_iters, got.refine_status, got.pass_res[:, 0] / (TOL * nb[0]), ratio, ra))
    assert got.refine_status == "out of iterations" and got.passes == 2
    assert got.pass_iters.tolist() == [plain.iters, extra] and got.iters == plain.iters + extra == len(got.res)
    assert np.all(ratio <= ra * (1 + 1e-6))
    worse = got.pass_res[2, 0] > got.pass_res[1, 0]
    if worse:                                                # the cut pass made it worse: xa itself comes back
        assert _same_bits(x, _cols(plain.x))
    cancel = (pb["n_max"] + 2) * U53 * np.linalg.norm(pb["absA0"] @ np.abs(x) + np.abs(B), axis=0) / np.linalg.norm(
        B - pb["A0"] @ x, axis=0)
    print("the cut pass made it %s; sys_res_original / (ratio ||b||) - 1 = %s, allowed %s" % (
        "worse" if worse else "better", got.sys_res_original / (ratio * nb) - 1, 2 * cancel))
    assert np.all(np.abs(got.sys_res_original - ratio * nb) <= 2 * cancel * ratio * nb)
    assert _same_bits(got.sys_res_original, got.pass_res[1 if worse else 2])
