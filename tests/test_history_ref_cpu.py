"""The references of the solution history check themselves, without a GPU (tests/history_ref.py): a float64 NumPy
restatement of project and append stays inside every bound the device test applies, every seeded mistake exceeds its
bound, and the facts about the sequences that tests/test_gpu_solution_history.py relies on hold for the restatement.

Problems as tests/test_gpu_system_solve.py builds them: P (= U) Poisson 10^3, G the graded S A0 S with its second
grading Gupd, E elasticity 12 x 10 x 10; right-hand sides default_rng(20260407).standard_normal((N, 16))."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import history_ref as H
from prealps_amd import gen

G_RANGE, G_RANGE_2 = (-2.0, 2.0), (1.0, -1.5)
TOL = 1e-5
_cache = {}


def matrix(name):
    if name in _cache:
        return _cache[name]
    if name == "E":
        rp, ci, v = gen.elasticity3d_csr((12, 10, 10))
    else:
        rp, ci, v = gen.poisson3d_csr(10)
        if name == "G":
            v = gen.graded_values(rp, ci, v, *G_RANGE)
        if name == "Gupd":
            v = gen.graded_values(rp, ci, v, *G_RANGE_2)
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    B = np.random.default_rng(20260407).standard_normal((N, 16))
    _cache[name] = dict(A=A, absA=abs(A), n_max=int(np.diff(rp).max()), N=N, B=B, lu=spla.splu(A.tocsc()))
    return _cache[name]


def solutions(pb, cols):
    return np.column_stack([pb["lu"].solve(pb["B"][:, j]) for j in cols])


def worst(pb, Hs, b, x0, kept, c, **kw):
    rho, bound = H.galerkin(pb["A"], pb["absA"], pb["n_max"], Hs.X, kept, b, x0, c, **kw)
    return float((np.abs(rho) / bound).max())


def filled(pb, cap=8, cols=range(5), **kw):
    Hs = H.RefHistory(cap, lambda X: np.asarray(pb["A"] @ X), **kw)
    Hs.append(solutions(pb, cols))
    return Hs


@pytest.mark.parametrize("name", ["P", "G", "E"])
def test_the_restatement_stays_inside_the_bounds(name):
    pb = matrix(name)
    Hs = filled(pb)
    b = pb["B"][:, 5]
    x0, rank, captured, kept, c, cs = Hs.project(b)
    assert rank == 5
    assert worst(pb, Hs, b, x0[:, 0], kept, c[:, 0]) <= 1.0
    # dots and combine against longdouble
    g = Hs.X.T @ pb["B"][:, 5:8]
    assert (np.abs(g - H.dots_exact(Hs.X, pb["B"][:, 5:8])) <= H.dots_bound(Hs.X, pb["B"][:, 5:8], pb["N"])).all()
    assert (np.abs(x0 - H.combine_exact(Hs.X, c)) <= H.combine_bound(Hs.X, c)).all()
    # the best approximation: closer to x* in the A-norm than zero and than every stored solution
    xs = pb["lu"].solve(b)
    e0 = H.energy_norm(pb["A"], xs - x0[:, 0])
    assert e0 <= H.energy_norm(pb["A"], xs)
    assert e0 <= min(H.energy_norm(pb["A"], xs - Hs.X[:, i]) for i in range(5)) * (1 + 1e-12)
    assert abs(captured[0] - H.energy_norm(pb["A"], x0[:, 0]) ** 2) <= 1e-9 * captured[0]


def test_a_dropped_tail_row_exceeds_the_bound():
    pb = matrix("P")
    Hs = filled(pb, dot=lambda X, W: X[:-1].T @ W[:-1])
    x0, _, _, kept, c, _ = Hs.project(pb["B"][:, 5])
    assert worst(pb, Hs, pb["B"][:, 5], x0[:, 0], kept, c[:, 0]) > 1.0


def test_a_column_read_at_the_wrong_ring_slot_exceeds_the_bound():
    pb = matrix("P")
    Hs = filled(pb)
    _, _, _, kept, c, _ = Hs.project(pb["B"][:, 5])
    x0 = np.roll(Hs.X, 1, axis=1) @ c[:, 0]
    assert worst(pb, Hs, pb["B"][:, 5], x0, kept, c[:, 0]) > 1.0


def test_a_scaling_multiplied_instead_of_divided_exceeds_the_bound():
    pb = matrix("G")
    d = np.sqrt(1.0 / np.maximum.reduceat(np.abs(pb["A"].data), pb["A"].indptr[:-1]))
    Hs = H.RefHistory(8, lambda X: (d * d)[:, None] * np.asarray(pb["A"] @ X))       # (A' x') * d in place of / d
    Hs.append(solutions(pb, range(5)))
    x0, _, _, kept, c, _ = Hs.project(pb["B"][:, 5])
    assert worst(pb, Hs, pb["B"][:, 5], x0[:, 0], kept, c[:, 0]) > 1.0


def test_a_stale_gram_matrix_after_a_values_change():
    """What the device test of the values update relies on: with G formed again the projection meets the bound of the
    new matrix, and misses that of the old one by more than 100 times; left stale it misses the new one."""
    old, new = matrix("G"), matrix("Gupd")
    Hs = filled(old)
    b = new["B"][:, 5]
    x0, _, _, kept, c, _ = Hs.project(b)
    assert worst(new, Hs, b, x0[:, 0], kept, c[:, 0]) > 1.0                 # stale
    Hs.matvec = lambda X: np.asarray(new["A"] @ X)
    Hs.refresh()
    x0, _, _, kept, c, _ = Hs.project(b)
    assert worst(new, Hs, b, x0[:, 0], kept, c[:, 0]) <= 1.0
    assert worst(old, Hs, b, x0[:, 0], kept, c[:, 0]) > 100.0


def test_an_evicted_row_that_is_not_removed_exceeds_the_bound():
    pb = matrix("P")
    X = solutions(pb, range(5))
    Hs = H.RefHistory(3, lambda V: np.asarray(pb["A"] @ V))
    for j in range(3):
        Hs.append(X[:, j])
    stale = Hs.G[0, 1:].copy()                      # the row of the column that the next append evicts
    Hs.append(X[:, 3])
    good = Hs.project(pb["B"][:, 5])
    assert worst(pb, Hs, pb["B"][:, 5], good[0][:, 0], good[3], good[4][:, 0]) <= 1.0
    Hs.G[2, :2] = Hs.G[:2, 2] = stale               # the new column's row still holds the evicted column's dots
    x0, _, _, kept, c, _ = Hs.project(pb["B"][:, 5])
    assert worst(pb, Hs, pb["B"][:, 5], x0[:, 0], kept, c[:, 0]) > 1.0
    # the ring itself: five appends at capacity 3 hold the last three, oldest first
    Hs = H.RefHistory(3, lambda V: np.asarray(pb["A"] @ V))
    Hs.append(X[:, :2]); Hs.append(X[:, 2:])
    assert Hs.count == 3 and np.array_equal(Hs.X, X[:, 2:])


@pytest.fixture(scope="module")
def heat():
    return H.heat_reference()


def test_the_heat_sequence_halves_the_iterations(heat):
    cold, hist = sum(heat["cold"][7:15]), sum(heat["hist"][7:15])
    print("steps 8..15: cold %d, history %d; per step %s" % (cold, hist, heat["hist"]))
    assert heat["cold"][0] == heat["hist"][0]                   # an empty history is the cold solve
    assert hist <= 0.5 * cold, (hist, cold)
    # the start residual of the projected start, relative to ||b||, over those steps
    rel = [g / n for g, n in zip(heat["g0"][7:15], heat["nb"][7:15])]
    assert max(rel) < 1e-2, rel


def test_a_repeated_right_hand_side_starts_converged_within_a_small_factor():
    """Solve b, then project b on a history that holds that solution alone: x0 = (x^T b / x^T A x) x, rank 1, and its
    residual is within 4 of the threshold the first solve stopped at (the device test allows 8)."""
    A, rowpos = H.heat_matrix()
    inv = [np.linalg.inv(A[r0:r1, r0:r1].toarray()) for r0, r1 in zip(rowpos[:-1], rowpos[1:])]
    b = np.random.default_rng(20260407).standard_normal((A.shape[0], 16))[:, :1]
    _, x, nb, _ = H.restate(A, rowpos, inv, b, 4, tol=TOL)
    Hs = H.RefHistory(8, lambda V: np.asarray(A @ V))
    Hs.append(x)
    x0, rank, _, _, _, _ = Hs.project(b)
    ratio = np.linalg.norm(b - A @ x0) / (TOL * nb[0])
    print("repeated right-hand side: start residual / (tol ||b||) = %.3f" % ratio)
    assert rank == 1 and ratio < 4.0
    hist2, _, _, _ = H.restate(A, rowpos, inv, b, 4, X0=x0, tol=TOL)
    assert len(hist2) <= 2
