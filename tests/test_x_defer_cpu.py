"""X every second row pass: the rule pa_ecg_x_mode (prealps_amd/csrc/ecg_plan.c) is plain host arithmetic.  A
stand-alone program (tests/c/x_defer_check.c) links the unit alone, is compiled with AddressSanitizer + UBSan and run as
a program, the way tests/test_ecg_plan_cpu.py runs the rest of the unit.  It prints the rule's answers, and the events of
simulated calls of the library's loops driven by the rule; what must hold of them is restated here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
EVERY, SKIP, BOTH = 0, 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/x_defer_check.c")
    tmp = tmp_path_factory.mktemp("x_defer")
    out, unit = str(tmp / "x_defer_check"), str(tmp / "ecg_plan.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "ecg_plan.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "x_defer_check.c"), unit, "-o", out])
    return out


def lines(exe, mode):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stderr[-4000:]
    return [line.split() for line in run.stdout.splitlines()]


def test_the_rule_over_all_eight_inputs(exe):
    got = {tuple(int(v) for v in row[:3]): int(row[3]) for row in lines(exe, "rule")}
    assert len(got) == 8
    for on in (0, 1):
        for pending in (0, 1):
            for ahead in (0, 1):
                want = BOTH if pending else (SKIP if on and ahead else EVERY)
                assert got[(on, pending, ahead)] == want, (on, pending, ahead)


def _check_events(on, events, stops):
    """events: the string of one case; stops: how many times the stopping test fired in it."""
    assert "?" not in events
    passes = re.sub(r"[^ESBF]", "", events)
    assert "SS" not in passes                                                  # no two skips without a payment between them
    assert "|1" not in events                                                  # nothing is owed at a return
    assert events.count("F") <= stops                                          # flushes only at stops
    for m in re.finditer("F", events):
        assert events[m.start() - 1] == "S"                                    # a flush pays the skip right before it
    # every skip is paid exactly once, by the next pass (B) or by a flush, before anything else happens
    for m in re.finditer("S", events):
        assert events[m.end():m.end() + 1] in ("B", "F"), events
    assert events.count("B") + events.count("F") == events.count("S")
    for m in re.finditer("B", events):
        assert events[m.start() - 1] == "S"
    if not on:
        assert set(passes) == {"E"} and "F" not in events


def test_simulated_advance_calls(exe):
    rows = lines(exe, "trace")
    seen = set()
    for on, n0, n1, n2, stop_at, events in rows:
        on, n, stop_at = int(on), (int(n0), int(n1), int(n2)), int(stop_at)
        seen.add((on, n, stop_at))
        _check_events(on, events, 1 if stop_at >= 0 else 0)
        calls = events.split("|")[:-1]          # (the text behind the last return mark is its 0)
        calls = [re.sub(r"^[01]", "", c) for c in calls]
        assert [len(re.sub("F", "", c)) for c in calls] == list(n)
        if on and stop_at < 0:
            # an unstopped call of k steps: k // 2 skips, an even one ends on BOTH, an odd one on EVERY; one step: EVERY
            for c, k in zip(calls, n):
                assert c == "SB" * (k // 2) + "E" * (k % 2), (c, k)
        if stop_at < 0:
            assert "F" not in events
    sizes = (1, 2, 3, 5)
    want = {(on, (a, b, c), s) for on in (0, 1) for a in sizes for b in sizes for c in sizes for s in range(-1, a + b + c)}
    assert seen == want


def test_simulated_solve(exe):
    rows = lines(exe, "solve")
    assert len(rows) == 18
    for on, stop_at, events in rows:
        on, stop_at = int(on), int(stop_at)
        _check_events(on, events, 1)
        if on:      # the stop after an odd number of steps falls on an owed update, after an even number it does not
            steps = stop_at + 1
            assert events == "SB" * (steps // 2) + ("SF" if steps % 2 else "") + "|0"
