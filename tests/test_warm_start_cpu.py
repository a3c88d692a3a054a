"""A start from an initial guess: what can be checked without a GPU -- the library exports the two entry points and
EcgProblem.solve / solve_multi refuse an impossible x0 / X0 before anything reaches the library."""
import numpy as np
import pytest

import prealps_amd as pa
import prealps_amd.lib as pl

GUESS = ("preAlps_ECGInitializeGuess", "preAlps_ECGSolveGuess")


@pytest.mark.parametrize("name", GUESS)
def test_library_exports_the_entry_point(name):
    L = pa.load()
    assert hasattr(L, name), name
    assert name in pl.EXPORTS


def _bare_problem(m):
    from prealps_amd.solver import EcgProblem
    prob = EcgProblem.__new__(EcgProblem)          # (no device, no operator: only the argument checks run)
    prob.m = m
    return prob


@pytest.mark.parametrize("x0", [np.zeros((12, 1)), np.zeros((12, 2, 1)), np.float64(1.0)])
def test_solve_refuses_an_x0_that_is_not_a_vector(x0):
    with pytest.raises(ValueError, match="x0 must be one-dimensional"):
        _bare_problem(12).solve(np.ones(12), 4, x0=x0)


def test_solve_refuses_the_wrong_row_count_of_x0():
    with pytest.raises(ValueError, match="x0 has 11 rows.*12 local rows"):
        _bare_problem(12).solve(np.ones(12), 4, x0=np.zeros(11))


@pytest.mark.parametrize("X0", [np.zeros(12), np.zeros((12, 2, 1)), np.float64(1.0)])
def test_solve_multi_refuses_an_x0_that_is_not_a_matrix(X0):
    with pytest.raises(ValueError, match="X0 must be two-dimensional"):
        _bare_problem(12).solve_multi(np.ones((12, 2)), 4, X0=X0)


def test_solve_multi_refuses_the_wrong_row_count_of_x0():
    with pytest.raises(ValueError, match="X0 has 11 rows.*12 local rows"):
        _bare_problem(12).solve_multi(np.ones((12, 2)), 4, X0=np.zeros((11, 2)))


@pytest.mark.parametrize("k,kx", [(2, 1), (2, 4), (4, 2), (1, 2)])
def test_solve_multi_refuses_another_column_count_than_b(k, kx):
    with pytest.raises(ValueError, match="X0 has %d columns, B has %d right-hand sides" % (kx, k)):
        _bare_problem(12).solve_multi(np.ones((12, k)), 4, X0=np.zeros((12, kx)))


def test_the_result_has_a_start_residual_field_that_defaults_to_none():
    from prealps_amd.solver import EcgResult
    r = EcgResult(x=None, iters=0, res=None, bs=None, final_res=0.0, final_bs=0, normb=0.0)
    assert r.sys_res0 is None
