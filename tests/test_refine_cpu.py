"""The stop decision of preAlps_ECGSolveSystemRefined (prealps_amd/csrc/ecg_refine.c) is plain host arithmetic: a
stand-alone program (tests/c/refine_verdict_check.c) links the unit alone, is compiled with AddressSanitizer + UBSan and
run as a program; the rule is restated here, independently of the C code.  And the switch of the operator's storage
without a device: preAlps_hip_set_operator_precision takes 64, 32 and 0, refuses everything else, works in plan-only
mode, and a bad PREALPS_SPMM_PRECISION is named by the next plan cut."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import prealps_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
CONTINUE, CONVERGED, OUT_OF_PASSES, OUT_OF_ITERATIONS, STAGNATED = -1, 0, 1, 2, 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/refine_verdict_check.c")
    tmp = tmp_path_factory.mktemp("ecg_refine")
    out, unit = str(tmp / "refine_verdict_check"), str(tmp / "ecg_refine.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "ecg_refine.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "refine_verdict_check.c"), unit, "-o", out, "-lm"])
    return out


def rows(exe, mode):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stderr[-4000:]
    return [line.split() for line in run.stdout.splitlines()]


def test_the_unit_is_pure_host_arithmetic():
    src = open(os.path.join(CSRC, "ecg_refine.c")).read() + open(os.path.join(CSRC, "ecg_refine.h")).read()
    includes = sorted(set(line.split()[1] for line in src.splitlines() if line.startswith("#include")))
    assert includes == ['"ecg_refine.h"', "<math.h>"]
    assert "getenv" not in src and "malloc" not in src and "static" not in src


def verdict(q, q_prev, p, max_passes, used, max_iter):
    """The rule of the issue, the first that applies: converged; out of iterations; a pass that does not halve
    max_j res_j / threshold_j; out of passes; else the pass runs."""
    keep = int(p >= 2 and q_prev < q)      # the chain ends unconverged: the better of the last two iterates
    if q <= 1.0:
        return CONVERGED, 0
    if used >= max_iter:
        return OUT_OF_ITERATIONS, keep
    if p >= 2 and (not (2.0 * q <= q_prev) or math.isinf(q)):      # (an infinite ratio is never "halved")
        return STAGNATED, keep
    if p >= max_passes:
        return OUT_OF_PASSES, keep
    return CONTINUE, 0


def test_ratio_one_system_and_several(exe):
    got = rows(exe, "ratio")
    assert len(got) == 8
    seen_k = set()
    for row in got:
        k = int(row[0])
        seen_k.add(k)
        vals = [float.fromhex(v) if v not in ("inf", "nan", "-nan") else float(v.lstrip("-")) for v in row[1:]]
        res, thr, q = vals[0:2 * k:2], vals[1:2 * k:2], vals[2 * k]
        with np.errstate(all="ignore"):
            quot = [np.float64(r) / np.float64(t) for r, t in zip(res, thr)]
        if any(not (x >= 0.0) or math.isinf(x) for x in quot):
            assert q == math.inf, row
        else:
            assert q == max(quot), row
    assert seen_k == {1, 2, 3, 4}
    # by hand: 3 / 2; 0; max(0.5, 2, 4); a NaN, an Inf, a zero threshold and a negative residual never pass
    assert [float.fromhex(r[-1]) if r[-1] != "inf" else math.inf for r in got[:7]] == [1.5, 0.0, 4.0, math.inf, math.inf,
                                                                                      math.inf, math.inf]


def test_every_verdict_and_the_halving_edge(exe):
    got = rows(exe, "verdict")
    tail, got = got[-1], got[:-1]
    assert tail == [str(STAGNATED)]                       # (keep_prev = NULL is allowed)
    assert len(got) == 10 * 7 * (1 + 2 + 4 + 16) * 4
    seen = set()
    for row in got:
        q, q_prev = (math.inf if v == "inf" else float.fromhex(v) for v in row[:2])
        p, mp, used, max_iter, v, keep = (int(x) for x in row[2:])
        assert (v, keep) == verdict(q, q_prev, p, mp, used, max_iter), row
        seen.add(v)
    assert seen == {CONTINUE, CONVERGED, OUT_OF_PASSES, OUT_OF_ITERATIONS, STAGNATED}
    def num(v):
        return math.inf if v == "inf" else float.fromhex(v)
    by = {(num(r[0]), num(r[1]), int(r[2]), int(r[3]), int(r[4])): (int(r[6]), int(r[7])) for r in got}
    above = lambda x: float(np.nextafter(x, math.inf))
    below = lambda x: float(np.nextafter(x, -math.inf))
    # the edge of the halving rule at pass 2 of 4, nothing used: q_prev = 4 -> q = 2 is halved, one ulp above is not
    assert by[2.0, 4.0, 2, 4, 0] == (CONTINUE, 0)
    assert by[above(2.0), 4.0, 2, 4, 0] == (STAGNATED, 0)
    assert by[below(2.0), 4.0, 2, 4, 0] == (CONTINUE, 0)
    assert by[2.0, above(4.0), 2, 4, 0] == (CONTINUE, 0)
    # worse than before: the earlier iterate is the better one
    assert by[3.0, 2.0, 2, 4, 0] == (STAGNATED, 1)
    # pass 1 has no predecessor to compare with; the last pass allowed has run
    assert by[1e3, 1.5, 1, 4, 0] == (CONTINUE, 0) and by[1e3, 1.5, 1, 1, 0] == (OUT_OF_PASSES, 0)
    # the budget counts before the rest; exactly 1 is converged, one ulp above is not
    assert by[3.0, 2.0, 2, 4, 100] == (OUT_OF_ITERATIONS, 1) and by[3.0, 2.0, 2, 4, 99] == (STAGNATED, 1)
    assert by[3.0, 6.0, 2, 4, 100] == (OUT_OF_ITERATIONS, 0) and by[3.0, 6.0, 1, 4, 100] == (OUT_OF_ITERATIONS, 0)
    assert by[1.0, 2.0, 2, 4, 101] == (CONVERGED, 0)
    assert by[above(1.0), 6.0, 4, 4, 0] == (OUT_OF_PASSES, 0)
    assert by[math.inf, 6.0, 2, 4, 0] == (STAGNATED, 1) and by[math.inf, math.inf, 2, 4, 0] == (STAGNATED, 0)


def test_chains_share_one_iteration_budget(exe):
    got = [[int(v) for v in r] for r in rows(exe, "chain")]
    # max_passes, max_iter, passes that ran, status, keep_prev, iterations used, iterations of every pass
    assert got == [
        [4, 100, 1, CONVERGED, 0, 30, 30],
        [4, 100, 2, CONVERGED, 0, 35, 30, 5],
        [1, 100, 1, OUT_OF_PASSES, 0, 30, 30],
        [3, 100, 3, OUT_OF_PASSES, 0, 30, 10, 10, 10],
        [4, 100, 3, CONTINUE, 0, 35, 30, 5, 0],
        [4, 100, 3, STAGNATED, 0, 40, 30, 5, 5],
        [4, 100, 2, STAGNATED, 1, 35, 30, 5],
        [4, 100, 2, OUT_OF_ITERATIONS, 0, 100, 60, 40],
        [16, 1000, 16, OUT_OF_PASSES, 0, 16] + [1] * 16,
        [4, 30, 1, OUT_OF_ITERATIONS, 0, 30, 30],
    ]


def test_passes_between_1_and_16(exe):
    assert {int(a): int(b) for a, b in rows(exe, "passes")} == {mp: int(1 <= mp <= 16) for mp in range(-1, 19)}


# ---- the switch, through ctypes, without a device --------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 32, 64])
def test_set_operator_precision_takes_64_32_and_0(bits):
    L = pa.load()
    try:
        assert L.preAlps_hip_set_operator_precision(bits) == 0
    finally:
        L.preAlps_hip_set_operator_precision(0)


@pytest.mark.parametrize("bits", [16, -1, 33])
def test_set_operator_precision_refuses_other_values(bits):
    L = pa.load()
    try:
        assert L.preAlps_hip_set_operator_precision(32) == 0
        assert L.preAlps_hip_set_operator_precision(bits) != 0
        msg = L.preAlps_hip_last_error().decode()
        assert "preAlps_hip_set_operator_precision" in msg and ("precision %d refused" % bits) in msg
    finally:
        L.preAlps_hip_set_operator_precision(0)


def _plan_only_problem():
    from oracle import oracle as O
    A = O.poisson3d(6)
    rp, ci, v = O.as_csr(A)
    return pa.EcgProblem(rp, ci, v, 4, O.contiguous_partition(A.shape[0], 4), scale=True, plan_only=True)


def test_the_switch_works_in_plan_only_mode_and_a_bad_variable_is_named_by_the_next_plan_cut(monkeypatch):
    monkeypatch.delenv("PREALPS_SPMM_PRECISION", raising=False)
    prob = _plan_only_problem()
    L = prob.L
    try:
        prob.set_operator_precision("single")
        prob.set_operator_precision("double")
        assert L.preAlps_hip_prepare_operator(4) == 0
        for good in ("single", "double", ""):
            monkeypatch.setenv("PREALPS_SPMM_PRECISION", good)
            assert L.preAlps_hip_set_operator_precision(0) == 0 and L.preAlps_hip_prepare_operator(4) == 0
        monkeypatch.setenv("PREALPS_SPMM_PRECISION", "half")
        assert L.preAlps_hip_set_operator_precision(0) == 0          # the setter does not read it ...
        assert L.preAlps_hip_prepare_operator(4) != 0                 # ... the plan cut does, and names it
        msg = L.preAlps_hip_last_error().decode()
        assert "PREALPS_SPMM_PRECISION=half" in msg and "double or single" in msg
        assert L.preAlps_hip_set_operator_precision(64) == 0          # a value given to the entry overrides the variable
        assert L.preAlps_hip_prepare_operator(4) == 0
    finally:
        prob.close()
    assert pa.load().preAlps_hip_set_operator_precision(0) == 0


def test_python_keywords_refuse_unknown_values():
    from prealps_amd.solver import EcgProblem
    prob = EcgProblem.__new__(EcgProblem)          # (no device: only the argument check runs)
    with pytest.raises(ValueError, match="precision"):
        prob.set_operator_precision("half")


def test_the_new_entries_are_declared_and_exported():
    L = pa.load()
    for name in ("preAlps_hip_set_operator_precision", "preAlps_ECGSolveSystemRefined"):
        assert name in pa.lib.EXPORTS and hasattr(L, name)
    assert pa.lib.REFINE_STATUS == {0: "converged", 1: "out of passes", 2: "out of iterations", 3: "stagnated"}
