"""The value map behind preAlps_OperatorUpdateValues (prealps_amd/csrc/spmm_plan.c: pa_spmm_plan_value_map): which
panel entry every stored value of an SpMM plan is.  tests/c/value_map_check.c, a stand-alone program built with
AddressSanitizer + UBSan like the plan dump of test_spmm_plan_cpu.py, holds it against the plan builders on that
dump's panels: nothing but `val` depends on the values, `val` is the gather the map describes, and every panel
entry is in it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")


@pytest.fixture(scope="module")
def check_lines(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/value_map_check.c")
    tmp = tmp_path_factory.mktemp("value_map")
    exe, unit = str(tmp / "value_map_check"), str(tmp / "spmm_plan.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "spmm_plan.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "value_map_check.c"), unit, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or map failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout.splitlines()


def _fields(line):
    head, rest = line.split(": ", 1)
    return head, dict(x.split("=", 1) for x in rest.split())


def test_the_map_is_the_gather_of_every_plan_kind(check_lines):
    """The program exits non-zero on any violation (the fixture asserts that); here: the cases still reach the
    window, the staged and the run plan, at every stride, on whole panels and on shards with halo slots."""
    cases = [_fields(l) for l in check_lines]
    assert len(cases) == 5 * 2 * 3 * 5            # panels x CU counts x strides x switch pairs
    for ts in (4, 8, 16):
        kinds = {f["kind"] for h, f in cases if " ts=%d " % ts in h}
        assert kinds == {"window", "staged", "runs"}, (ts, kinds)
    for panel in ("poisson12", "nodes8", "random2048", "poisson12_shard", "nodes8_shard"):
        assert any(h.startswith(panel + " ") for h, _ in cases)
    assert {f["kind"] for h, f in cases if h.startswith("poisson12_shard ")} == {"window", "staged", "runs"}
    assert all(int(f["slots"]) % 64 == 0 and int(f["slots"]) >= int(f["entries"]) for _, f in cases)


def test_window_and_staged_plans_hold_every_entry_once(check_lines):
    for h, f in (_fields(l) for l in check_lines):
        if f["kind"] != "runs":
            assert f["repeated"] == "0", h
