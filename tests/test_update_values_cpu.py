"""preAlps_OperatorUpdateValues on the host (plan-only mode, no GPU): new values for the same pattern give the row
panel that a fresh build from them gives, bit for bit, at the same address; every refusal leaves the operator as it
was; op_values_epoch counts the updates that went through."""
import ctypes as C
import os

import numpy as np
import pytest

import prealps_amd
from prealps_amd import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix(kind):
    if kind == "poisson":
        rp, ci, v = gen.poisson3d_csr(10)
        part, P = gen.box_partition(10, (5, 5, 5))
        assert P == 8
    else:
        nn = (12, 10, 10)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, P = gen.box_partition_nodes(nn, (2, 2, 2))
    return rp, ci, v, part, P


def _new_values(rp, ci, v):
    """v2 = S A S with S = diag(1 + 0.3 (2u - 1)): same pattern, still SPD (a congruence), every value and the
    scaling vector change."""
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    rows = np.repeat(np.arange(N), np.diff(rp))
    return s[rows] * v * s[ci]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _val_address(prob):
    return C.cast(prob.A.val, C.c_void_p).value


@pytest.fixture
def world():
    """set_world(rank, size) for a test, one process again afterwards."""
    L = prealps_amd.load()
    yield lambda rank, size: prealps_amd.lib.check(L.preAlps_hip_set_world(rank, size), "preAlps_hip_set_world")
    L.preAlps_hip_set_world(0, 1)
    L.preAlps_hip_plan_only(0)


@pytest.mark.parametrize("rank,size", [(0, 1), (1, 3)], ids=["one-process", "rank1of3"])
@pytest.mark.parametrize("scale", [True, False], ids=["scaled", "unscaled"])
@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_updated_panel_is_the_fresh_build_in_bits(kind, scale, rank, size, world):
    rp, ci, v, part, P = _matrix(kind)
    v2 = _new_values(rp, ci, v)
    assert np.all(v2[v != 0.0] != v[v != 0.0])           # (the elasticity pattern stores some zeros)
    world(rank, size)
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=scale, plan_only=True)
    try:
        rp0, ci0, v0 = prob.local_csr()
        addr = _val_address(prob)
        assert prob.stat("op_values_epoch") == 0
        prob.update_values(v2)
        assert prob.stat("op_values_epoch") == 1
        assert _val_address(prob) == addr                  # the struct copy the caller holds stays valid ...
        A = prealps_amd.CPLM_Mat_CSR_t()
        prealps_amd.lib.check(prob.L.preAlps_OperatorGetA(C.byref(A)), "preAlps_OperatorGetA")
        assert C.cast(A.val, C.c_void_p).value == addr     # ... and is what the library hands out
        rp1, ci1, v1 = prob.local_csr()
    finally:
        prob.close()
    world(rank, size)
    fresh = prealps_amd.EcgProblem(rp, ci, v2, P, part, scale=scale, plan_only=True)
    try:
        rpf, cif, vf = fresh.local_csr()
        assert fresh.stat("op_values_epoch") == 0          # a build starts the count again
    finally:
        fresh.close()
    assert np.array_equal(rp1, rp0) and np.array_equal(ci1, ci0)
    assert np.array_equal(rp1, rpf) and np.array_equal(ci1, cif)
    assert len(v1) == len(vf) and len(v1) > 0
    assert np.array_equal(_bits(v1), _bits(vf))
    assert not np.array_equal(_bits(v1), _bits(v0))
    if size > 1:
        assert len(v1) < len(v)                             # a shard: part of the rows only


def test_an_update_can_be_undone_in_bits(world):
    rp, ci, v, part, P = _matrix("poisson")
    v2 = _new_values(rp, ci, v)
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, plan_only=True)
    try:
        v0 = prob.local_csr()[2]
        prob.update_values(v2)
        prob.update_values(v)
        assert np.array_equal(_bits(prob.local_csr()[2]), _bits(v0))
        assert prob.stat("op_values_epoch") == 2
        assert prob.stat("op_value_map_builds") == 0 and prob.stat("op_value_map_bytes") == 0   # no plan, no map
    finally:
        prob.close()


def test_refusals_name_the_entry_and_leave_the_operator_alone(world):
    L = prealps_amd.load()
    pd = C.POINTER(C.c_double)
    rp, ci, v, part, P = _matrix("poisson")
    v2 = _new_values(rp, ci, v)

    def refused(ptr, *words):
        assert L.preAlps_OperatorUpdateValues(ptr) != 0
        msg = L.preAlps_hip_last_error()
        assert b"preAlps_OperatorUpdateValues" in msg, msg
        for w in words:
            assert w in msg, msg

    L.preAlps_OperatorFree()
    refused(v2.ctypes.data_as(pd), b"not built")                                   # no operator
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, plan_only=True)
    try:
        prob.update_values(v2)
        before = prob.local_csr()[2]
        refused(None, b"val != NULL")                                              # NULL
        with pytest.raises(prealps_amd.PreAlpsError, match="preAlps_OperatorUpdateValues"):
            prob.update_values(None)
        with pytest.raises(ValueError):
            prob.update_values(v2[:-1])
        with pytest.raises(ValueError):
            prob.update_values(v2, precond="lag")
        v3 = v.copy()                                                              # a zero row under scaling
        v3[rp[len(rp) // 2]:rp[len(rp) // 2 + 1]] = 0.0
        refused(v3.ctypes.data_as(pd), b"Impossible to scale the matrix, rcmin=0")
        with pytest.raises(prealps_amd.PreAlpsError, match="rcmin=0"):
            prob.update_values(v3)
        assert np.array_equal(_bits(prob.local_csr()[2]), _bits(before))           # the old values are in place
        assert prob.stat("op_values_epoch") == 1                                   # successful updates only
        prob.update_values(v)
        assert prob.stat("op_values_epoch") == 2
    finally:
        prob.close()
    # the same zero row is no error without scaling: the values are taken as they are
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=False, plan_only=True)
    try:
        prob.update_values(v3)
        assert prob.stat("op_values_epoch") == 1
    finally:
        prob.close()


def test_an_operator_read_from_a_file_is_refused(world, monkeypatch):
    L = prealps_amd.load()
    monkeypatch.setenv("PREALPS_NPARTS", "2")
    monkeypatch.setenv("PREALPS_PARTITION", "contiguous")
    L.preAlps_hip_plan_only(1)
    try:
        mtx = os.path.join(ROOT, "tests", "golden", "LFAT5.mtx")
        prealps_amd.lib.check(L.preAlps_OperatorBuild(mtx.encode(), 0x44000000), "preAlps_OperatorBuild")
        A = prealps_amd.CPLM_Mat_CSR_t()
        prealps_amd.lib.check(L.preAlps_OperatorGetA(C.byref(A)), "preAlps_OperatorGetA")
        nnz = A.info.lnnz
        before = np.ctypeslib.as_array(A.val, shape=(nnz,)).copy()
        vals = np.ones(nnz)
        assert L.preAlps_OperatorUpdateValues(vals.ctypes.data_as(C.POINTER(C.c_double))) != 0
        msg = L.preAlps_hip_last_error()
        assert b"preAlps_OperatorUpdateValues" in msg and b"file" in msg, msg
        assert np.array_equal(np.ctypeslib.as_array(A.val, shape=(nnz,)), before)
        v = C.c_double(-1.0)
        assert L.preAlps_hip_get_stat(b"op_values_epoch", C.byref(v)) == 0 and v.value == 0
    finally:
        L.preAlps_OperatorFree()
        L.preAlps_hip_plan_only(0)
