"""Several right-hand sides: what can be checked without a GPU -- the library exports the entry points and
EcgProblem.solve_multi refuses impossible shapes before anything reaches the library."""
import numpy as np
import pytest

import prealps_amd as pa
import prealps_amd.lib as pl

MULTI = ("preAlps_ECGInitializeMulti", "preAlps_ECGSystemResiduals", "preAlps_ECGFinalizeMulti",
         "preAlps_ECGSolveMulti")


@pytest.mark.parametrize("name", MULTI)
def test_library_exports_the_entry_point(name):
    L = pa.load()
    assert hasattr(L, name), name
    assert name in pl.EXPORTS


def _bare_problem(m):
    from prealps_amd.solver import EcgProblem
    prob = EcgProblem.__new__(EcgProblem)          # (no device, no operator: only the argument checks run)
    prob.m = m
    return prob


@pytest.mark.parametrize("B", [np.zeros(12), np.zeros((12, 2, 1)), np.float64(1.0)])
def test_solve_multi_refuses_what_is_not_a_matrix(B):
    with pytest.raises(ValueError, match="two-dimensional"):
        _bare_problem(12).solve_multi(B, 4)


def test_solve_multi_refuses_the_wrong_row_count():
    with pytest.raises(ValueError, match="11 rows.*12 local rows"):
        _bare_problem(12).solve_multi(np.zeros((11, 2)), 4)


@pytest.mark.parametrize("k,t", [(3, 4), (2, 3), (4, 2), (5, 16)])
def test_solve_multi_refuses_t_that_is_no_multiple_of_k(k, t):
    with pytest.raises(ValueError, match="not a multiple"):
        _bare_problem(12).solve_multi(np.ones((12, k)), t)


def test_solve_multi_refuses_no_right_hand_side():
    with pytest.raises(ValueError, match="not a multiple"):
        _bare_problem(12).solve_multi(np.ones((12, 0)), 4)
