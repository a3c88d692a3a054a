"""The solution history on several processes, what needs no GPU: the layout of the buffer one all-reduce of an entry
carries (pa_hist_red_layout in prealps_amd/csrc/ecg_history.c), run as a stand-alone program (tests/c/history_red_check.c)
under AddressSanitizer + UBSan as tests/test_ecg_history_cpu.py runs history_check.c, and the argument checks of
EcgProblem.solve_system(history=True), which come before any library call.

The layout, restated: the buffer has 1 + 16 + 256 + 256 words, [failed | 16 sums | first block | second block]; a block
is column major with the leading dimension of its rows and starts where its region starts:
  project  b_0^2 .. b_q-1^2 at word 1, g (K x q) at word 17; 273 words travel     K in 0 .. 16, q in 1 .. 16
  append   DO (K x q) at word 17, DN (q x q) at word 273; 529 words travel        K in 0 .. 16, q in 1 .. 16
  refresh  G (K x K) at word 17; 273 words travel                                 K in 1 .. 16
so neither the place of an entry (i, j) nor the word count depends on q."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
PROJECT, APPEND, REFRESH = 0, 1, 2
WORDS = 1 + 16 + 256 + 256


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/history_red_check.c")
    tmp = tmp_path_factory.mktemp("history_red")
    out, unit = str(tmp / "history_red_check"), str(tmp / "ecg_history.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "ecg_history.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "history_red_check.c"), unit, "-o", out, "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    got = subprocess.run([out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert got.returncode == 0 and got.stderr == "", "sanitizer or program failure (%d):\n%s" % (got.returncode, got.stderr[-4000:])
    return {tuple(int(w) for w in line.split()[:3]): [int(w) for w in line.split()[3:]] for line in got.stdout.splitlines()}


def _expected(entry, K, q):
    """(off_a, rows_a, cols_a, off_b, rows_b, cols_b, words), or None where the shape is refused."""
    if entry == REFRESH:
        return (17, K, K, 273, 0, 0, 273) if 1 <= K <= 16 else None
    if entry not in (PROJECT, APPEND) or not (0 <= K <= 16 and 1 <= q <= 16):
        return None
    if entry == PROJECT:
        return (1, 1, q, 17, K, q, 273)
    return (17, K, q, 273, q, q, WORDS)


def test_every_shape_has_the_stated_layout_and_refused_shapes_are_refused(lines):
    assert len(lines) == 5 * 19 * 19
    for (entry, K, q), got in lines.items():
        want = _expected(entry, K, q)
        if want is None:
            assert got == [1], (entry, K, q, got)            # PA_HIST_BAD_ARGS, and nothing else printed
        else:
            assert got == [0] + list(want), (entry, K, q, got)


def test_the_blocks_lie_apart_behind_word_0_and_inside_the_buffer(lines):
    largest = 0
    for entry in (PROJECT, APPEND, REFRESH):
        for K in range(1, 17):
            for q in range(1, 17):
                st, off_a, ra, ca, off_b, rb, cb, words = lines[(entry, K, q)]
                assert st == 0
                a = set(range(off_a, off_a + ra * ca))
                b = set(range(off_b, off_b + rb * cb))
                assert not (a & b) and 0 not in a and 0 not in b
                assert a | b <= set(range(1, words)) and words <= WORDS
                largest = max(largest, max(a | b))
    assert largest == WORDS - 1                              # an append of 16 columns: the last word of DN


def test_the_unit_stays_pure_host_arithmetic():
    src = open(os.path.join(CSRC, "ecg_history.c")).read() + open(os.path.join(CSRC, "ecg_history.h")).read()
    includes = sorted(set(line.split()[1] for line in src.splitlines() if line.startswith("#include")))
    assert includes == ['"ecg_history.h"', "<math.h>"]
    assert "getenv" not in src and "malloc" not in src and "static" not in src
    assert "pa_hist_red_layout" in src


def test_history_true_refuses_x0_refine_and_energy_before_any_library_call():
    import prealps_amd
    from prealps_amd import gen
    rp, ci, v = gen.poisson3d_csr(6)
    prob = prealps_amd.EcgProblem(rp, ci, v, 4, None, scale=True, plan_only=True)
    try:
        b = np.ones(prob.N)
        calls = []
        real = prob.L

        class Spy:
            def __getattr__(self, name):
                calls.append(name)
                return getattr(real, name)

        prob.L = Spy()
        try:
            for kw in (dict(x0=b), dict(refine=True), dict(energy=True), dict(stop="energy")):
                with pytest.raises(ValueError, match="history=True"):
                    prob.solve_system(b, 4, history=True, **kw)
            assert calls == []
        finally:
            prob.L = real
    finally:
        prob.close()
        prealps_amd.load().preAlps_hip_plan_only(0)
