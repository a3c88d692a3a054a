"""pa_ecg_switch_t.ride_sys (prealps_amd/csrc/ecg_plan.c): the caller's stopping metric on several processes lets its
per-system sums ride on a collective of the iteration.  A stand-alone program (tests/c/ecg_plan_ride_check.c) links the
unit alone under AddressSanitizer + UBSan and prints, for every input of the switch table, the eight decisions; the
rules are restated here, independently of the C code and of tests/test_ecg_plan_cpu.py."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
ORTHOMIN, ORTHODIR, ORTHODIR_FUSED = 0, 1, 2
ADAPT_BS, NO_BS_RED = 0, 1


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/ecg_plan_ride_check.c")
    tmp = tmp_path_factory.mktemp("ecg_plan_ride")
    out, unit = str(tmp / "ecg_plan_ride_check"), str(tmp / "ecg_plan.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "ecg_plan.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "ecg_plan_ride_check.c"), unit, "-o", out])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stderr[-4000:]
    return [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]


def seven_switches(alg, bs_red, enlFac, nrhs, guess, metric, world, loopback, timing, fuse, lazy_norm_sw, lazy_stop_sw,
                   graphs, poll_sw):
    """expected_switches of tests/test_ecg_plan_cpu.py, restated."""
    several = nrhs > 1 or guess or metric
    rotate = bs_red == NO_BS_RED
    lazy_norm = bool(fuse and alg == ORTHODIR and lazy_norm_sw)
    lazy_stop = bool(fuse and rotate and alg != ORTHODIR_FUSED and enlFac >= 2 and lazy_stop_sw)
    request = 0 if several else graphs
    use_graphs = bool(request and (world == 1 or loopback or request == 2) and rotate and fuse and alg != ORTHODIR_FUSED
                      and not timing)
    if use_graphs:
        lazy_stop = False
    poll = bool((poll_sw != 0 if poll_sw >= 0 else world > 1) and not use_graphs and not several)
    ride = nrhs > 1 and not metric and world > 1
    return tuple(int(v) for v in (rotate, fuse, lazy_norm, lazy_stop, use_graphs, poll, ride))


def test_ride_sys_is_the_callers_metric_on_several_processes(table):
    want_inputs = set(itertools.product([ORTHOMIN, ORTHODIR, ORTHODIR_FUSED], [ADAPT_BS, NO_BS_RED], [1, 2, 4, 8], [1, 2],
                                        [0, 1], [0, 1], [(1, 0), (1, 1), (8, 0)], [0, 1], [0, 1], [0, 1], [0, 1], [0, 1, 2],
                                        [-1, 0, 1]))
    assert len(table) == len(want_inputs) == 82944
    seen, on = set(), 0
    for row in table:
        assert len(row) == 22
        i = row[:14]
        seen.add(i[:6] + ((i[6], i[7]),) + i[8:])
        metric, world = i[5], i[6]
        assert row[21] == int(bool(metric and world > 1)), row          # ride_sys, whatever nrhs
        assert row[14:21] == seven_switches(*i), row                    # the seven in front of it are unchanged
        assert not (row[20] and row[21]), row                           # ride and ride_sys exclude each other
        on += row[21]
    assert seen == want_inputs
    assert on == 82944 // 2 // 3                                        # metric = 1 and the one world of 8
