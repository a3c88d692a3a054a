"""The host side of the system solve (preAlps_ECGSolveSystem), in plan-only mode, without a GPU: the operator keeps
its scaling vector -- d_i = sqrt(1 / max_j |a_ij|) in the caller's order, at one address for the operator's life --
and EcgProblem.solve_system refuses bad arguments before any library call.

Problems: P = Poisson 10^3 with part[i] = (i // 5) % 8, a partition that is not contiguous, so perm is far from the
identity; G = the graded S A0 S, S = diag(10^linspace(-2, 2, N)), on 8 contiguous parts; E = elasticity on 12 x 10 x 10
nodes with boxes of 2 x 2 x 2 nodes; U = P built with scale=False."""
import ctypes as C

import numpy as np
import pytest

import prealps_amd
from prealps_amd import gen


def _matrix(name):
    if name in ("P", "U"):
        rp, ci, v = gen.poisson3d_csr(10)
        return rp, ci, v, ((np.arange(1000) // 5) % 8).astype(np.int32), 8
    if name == "G":
        rp, ci, v = gen.poisson3d_csr(10)
        return rp, ci, gen.graded_values(rp, ci, v, -2.0, 2.0), None, 8
    nn = (12, 10, 10)
    rp, ci, v = gen.elasticity3d_csr(nn)
    part, P = gen.box_partition_nodes(nn, (2, 2, 2))
    return rp, ci, v, part, P


def _problem(name):
    rp, ci, v, part, P = _matrix(name)
    return prealps_amd.EcgProblem(rp, ci, v, P, part, scale=name != "U", plan_only=True), rp, ci, v


def _row_scaling(rp, v):
    """order_and_scale's d from its definition, with the library's operations: sqrt(1.0 / max)."""
    return np.sqrt(1.0 / np.maximum.reduceat(np.abs(v), rp[:-1]))


def _scaling_address(prob):
    d, n = C.POINTER(C.c_double)(), C.c_int()
    prealps_amd.lib.check(prob.L.preAlps_OperatorGetScalingPtr(C.byref(d), C.byref(n)), "preAlps_OperatorGetScalingPtr")
    return C.cast(d, C.c_void_p).value, n.value


@pytest.fixture(autouse=True)
def _one_process_again():
    yield
    L = prealps_amd.load()
    L.preAlps_hip_set_world(0, 1)
    L.preAlps_hip_plan_only(0)


def test_the_new_symbols_are_exported():
    L = prealps_amd.load()
    for name in ("preAlps_OperatorGetScalingPtr", "preAlps_ECGSolveSystem", "preAlps_OperatorSystemResiduals"):
        assert name in prealps_amd.lib.EXPORTS and hasattr(L, name)
    assert (prealps_amd.lib.SYS_DEVICE, prealps_amd.lib.SYS_STOP_ORIGINAL) == (1, 2)


@pytest.mark.parametrize("name", ["P", "G", "E"])
def test_scaling_is_the_row_scaling_in_the_callers_order(name):
    prob, rp, ci, v = _problem(name)
    try:
        d = prob.scaling
        assert d.shape == (prob.N,) and d.dtype == np.float64
        assert d.tobytes() == _row_scaling(rp, v).tobytes()
        # the host panel is P D A D P^T: row i of it is the caller's row perm[i], entry by entry, in the library's order
        # of operations (d[row] * a) * d[col]
        perm = prob.perm
        lrp, lci, lv = prob.local_csr()
        import scipy.sparse as sp
        A = sp.csr_matrix((v, ci, rp), shape=(prob.N, prob.N))
        A.sort_indices()
        rows = np.repeat(np.arange(prob.m), np.diff(lrp))
        old_r, old_c = perm[rows], perm[lci]
        a = np.asarray(A[old_r, old_c]).ravel()
        assert lv.tobytes() == ((d[old_r] * a) * d[old_c]).tobytes()
        assert prob.stat("op_system_map_builds") == 0 and prob.stat("op_system_map_bytes") == 0
    finally:
        prob.close()


def test_an_unscaled_problem_has_no_scaling():
    prob, rp, ci, v = _problem("U")
    try:
        assert prob.scaling is None
        assert _scaling_address(prob) == (None, prob.N)
    finally:
        prob.close()


def test_scaling_for_any_world_size():
    L = prealps_amd.load()
    rp, ci, v, part, P = _matrix("E")
    prealps_amd.lib.check(L.preAlps_hip_set_world(1, 3), "preAlps_hip_set_world")
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, plan_only=True)
    try:
        assert prob.m < prob.N
        assert prob.scaling.tobytes() == _row_scaling(rp, v).tobytes()
    finally:
        prob.close()


def test_an_update_writes_the_new_vector_at_the_same_address():
    prob, rp, ci, v = _problem("G")
    try:
        addr, n = _scaling_address(prob)
        assert addr and n == prob.N
        v2 = gen.graded_values(rp, ci, gen.poisson3d_csr(10)[2], 1.0, -1.5)
        prob.update_values(v2)
        assert _scaling_address(prob) == (addr, n)
        assert prob.scaling.tobytes() == _row_scaling(rp, v2).tobytes()
        assert prob.scaling.tobytes() != _row_scaling(rp, v).tobytes()
        # a refused update (a zero row) leaves the vector of the last accepted values
        bad = v2.copy()
        bad[rp[17]:rp[18]] = 0.0
        with pytest.raises(prealps_amd.PreAlpsError, match="rcmin=0"):
            prob.update_values(bad)
        assert _scaling_address(prob) == (addr, n)
        assert prob.scaling.tobytes() == _row_scaling(rp, v2).tobytes()
    finally:
        prob.close()


def test_solve_system_refuses_bad_arguments_before_any_library_call():
    prob, rp, ci, v = _problem("P")
    try:
        N = prob.N
        b = np.ones(N)
        B = np.ones((N, 2))
        with pytest.raises(ValueError, match="stop must be"):
            prob.solve_system(b, 4, stop="relative")
        with pytest.raises(ValueError, match="shape"):
            prob.solve_system(np.ones(N - 1), 4)
        with pytest.raises(ValueError, match="shape"):
            prob.solve_system(np.ones((N, 2, 1)), 4)
        with pytest.raises(ValueError, match="shape"):
            prob.solve_system(B, 4, x0=np.ones(N))
        with pytest.raises(ValueError, match="shape"):
            prob.solve_system(b, 4, x0=np.ones((N, 2)))
        with pytest.raises(ValueError, match="not a multiple"):
            prob.solve_system(np.ones((N, 3)), 4)
        with pytest.raises(ValueError, match="shape"):
            prob.system_residuals(B, np.ones((N, 3)))
        import torch
        with pytest.raises(ValueError, match="CPU tensor"):
            prob.solve_system(torch.ones(N, dtype=torch.float64), 4)
        with pytest.raises(ValueError, match="float64"):
            prob.solve_system(torch.ones(N, dtype=torch.float32), 4)
        # nothing of the above reached the library: no solver was asked for a device
        assert prob.stat("op_system_map_builds") == 0
    finally:
        prob.close()
