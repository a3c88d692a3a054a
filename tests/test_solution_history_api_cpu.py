"""The solution history without a GPU: the library exports its six entries, EcgProblem.solve_system(history=True)
refuses what does not go with it before any library call, the stats are 0 without a history, and the entries are
refused -- naming themselves -- without an operator, in plan-only mode and for a process group of several."""
import ctypes as C

import numpy as np
import pytest

import prealps_amd
from prealps_amd import gen

ENTRIES = ("preAlps_SolutionHistoryCreate", "preAlps_SolutionHistoryFree", "preAlps_SolutionHistoryClear",
           "preAlps_SolutionHistoryAppend", "preAlps_SolutionHistoryProject", "preAlps_ECGSolveSystemHistory")
STATS = ("hist_capacity", "hist_columns", "hist_bytes", "hist_appends", "hist_projections", "hist_last_rank",
         "hist_gram_refreshes", "hist_values_epoch")


def _problem():
    rp, ci, v = gen.poisson3d_csr(6)
    return prealps_amd.EcgProblem(rp, ci, v, 4, None, scale=True, plan_only=True)


@pytest.fixture(autouse=True)
def _one_process_again():
    yield
    L = prealps_amd.load()
    L.preAlps_hip_set_world(0, 1)
    L.preAlps_hip_plan_only(0)


def _last_error(L):
    return (L.preAlps_hip_last_error() or b"").decode()


def test_the_six_symbols_are_exported():
    L = prealps_amd.load()
    for name in ENTRIES:
        assert name in prealps_amd.lib.EXPORTS and hasattr(L, name), name


def test_stats_are_zero_without_a_history():
    L = prealps_amd.load()
    v = C.c_double(-1.0)
    for key in STATS:                         # without an operator
        assert L.preAlps_hip_get_stat(key.encode(), C.byref(v)) == 0 and v.value == 0.0, key
    prob = _problem()
    try:
        for key in STATS:
            assert prob.stat(key) == 0.0, key
        with pytest.raises(KeyError):
            prob.stat("hist_no_such_key")
    finally:
        prob.close()


def test_solve_system_with_history_refuses_what_does_not_go_with_it():
    prob = _problem()
    try:
        b = np.ones(prob.N)
        for kw in (dict(x0=np.ones(prob.N)), dict(refine=True), dict(energy=True), dict(stop="energy")):
            with pytest.raises(ValueError, match="history=True"):
                prob.solve_system(b, 4, history=True, **kw)
        with pytest.raises(ValueError, match="shape"):
            prob.history_project(np.ones(prob.N - 1))
        with pytest.raises(ValueError, match="shape"):
            prob.history_append(np.ones((prob.N, 2, 1)))
        import torch
        with pytest.raises(ValueError, match="CPU tensor"):
            prob.history_append(torch.ones(prob.N, dtype=torch.float64))
        assert prob.stat("op_system_map_builds") == 0 and prob.stat("hist_appends") == 0
    finally:
        prob.close()


def _call_all(L, e, buf, n):
    rank = C.c_int(-7)
    return {
        "preAlps_SolutionHistoryCreate": lambda: L.preAlps_SolutionHistoryCreate(8),
        "preAlps_SolutionHistoryClear": lambda: L.preAlps_SolutionHistoryClear(),
        "preAlps_SolutionHistoryAppend": lambda: L.preAlps_SolutionHistoryAppend(1, buf.ctypes.data, n, 0),
        "preAlps_SolutionHistoryProject": lambda: L.preAlps_SolutionHistoryProject(1, buf.ctypes.data, n, buf.ctypes.data, n, 0,
                                                                                 0.0, C.byref(rank), None),
        "preAlps_ECGSolveSystemHistory": lambda: L.preAlps_ECGSolveSystemHistory(C.byref(e), 1, buf.ctypes.data, n,
                                                                               buf.ctypes.data, n, 0, 0.0, None, None, None,
                                                                               None, None, None, C.byref(rank), 0, None),
    }


def test_refused_without_an_operator():
    L = prealps_amd.load()
    L.preAlps_OperatorFree()
    e, buf = prealps_amd.lib.preAlps_ECG_t(), np.ones(8)
    for name, call in _call_all(L, e, buf, 8).items():
        assert call() != 0, name
        msg = _last_error(L)
        assert msg.startswith(name + ":") and "operator must be built" in msg, msg
    assert L.preAlps_SolutionHistoryFree() == 0          # nothing to free is no error


def test_refused_in_plan_only_mode_and_for_several_processes():
    prob = _problem()
    L = prob.L
    try:
        e, buf = prob.new_ecg(4), np.ones(prob.N)
        for name, call in _call_all(L, e, buf, prob.N).items():
            assert call() != 0, name
            msg = _last_error(L)
            assert msg.startswith(name + ":") and "plan-only" in msg, msg
        with pytest.raises(prealps_amd.PreAlpsError, match="preAlps_SolutionHistoryCreate.*plan-only"):
            prob.enable_history(8)
        with pytest.raises(prealps_amd.PreAlpsError, match="preAlps_ECGSolveSystemHistory"):
            prob.has_precond = True       # (plan-only: no factor is created; the entry must refuse on its own)
            prob.solve_system(buf, 4, history=True)
        for key in STATS:
            assert prob.stat(key) == 0.0, key
    finally:
        prob.has_precond = False
        prob.close()
    rp, ci, v = gen.poisson3d_csr(6)
    prealps_amd.lib.check(L.preAlps_hip_set_world(1, 2), "preAlps_hip_set_world")
    prob = prealps_amd.EcgProblem(rp, ci, v, 4, None, scale=True, plan_only=True)
    try:
        L.preAlps_hip_plan_only(0)
        assert L.preAlps_SolutionHistoryCreate(8) != 0
        msg = _last_error(L)
        assert msg.startswith("preAlps_SolutionHistoryCreate:") and "single process" in msg, msg
    finally:
        L.preAlps_hip_plan_only(1)
        prob.close()
