"""preAlps_BlockJacobiUpdateValues without a GPU: the entry is exported and declared, and
EcgProblem.update_values(val, precond="refactor") in plan-only mode, where no preconditioner exists, updates the
panel like "rebuild" does and raises nothing; other strings are still refused."""
import os
import re

import numpy as np
import pytest

import prealps_amd
from prealps_amd import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "preAlps_BlockJacobiUpdateValues"


def test_the_entry_is_exported_and_declared():
    L = prealps_amd.load()
    assert hasattr(L, ENTRY) and ENTRY in prealps_amd.lib.EXPORTS
    txt = open(os.path.join(ROOT, "include", "preAlps_hip.h")).read()
    assert re.search(r"^int %s\(void\);" % ENTRY, re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.M)
    assert hasattr(prealps_amd.EcgProblem, "refactor_block_jacobi")


def test_refused_without_a_preconditioner_and_without_a_gpu():
    L = prealps_amd.load()
    L.preAlps_BlockJacobiFree()
    assert L.preAlps_BlockJacobiUpdateValues() != 0
    msg = L.preAlps_hip_last_error()
    assert ENTRY.encode() in msg and b"not created" in msg, msg


def test_refactor_without_a_preconditioner_updates_the_panel_only():
    rp, ci, v = gen.poisson3d_csr(10)
    part, P = gen.box_partition(10, (5, 5, 5))
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    v2 = s[np.repeat(np.arange(N), np.diff(rp))] * v * s[ci]
    L = prealps_amd.load()
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, plan_only=True)
    try:
        before = prob.local_csr()[2]
        prob.update_values(v2, precond="refactor")
        assert prob.stat("op_values_epoch") == 1 and not prob.has_precond
        assert prob.stat("bj_updates") == 0 and prob.stat("bj_band_map_builds") == 0
        after = prob.local_csr()[2]
        assert not np.array_equal(after, before)
        prob.update_values(v2, precond="rebuild")
        assert np.array_equal(prob.local_csr()[2].view(np.uint64), after.view(np.uint64))
        with pytest.raises(ValueError):
            prob.update_values(v2, precond="lag")
        assert prob.stat("op_values_epoch") == 2
    finally:
        prob.close()
        L.preAlps_hip_plan_only(0)
