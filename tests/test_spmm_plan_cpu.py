"""The SpMM plan builders (prealps_amd/csrc/spmm_plan.c) are host arithmetic on a CSR panel: a
stand-alone program cuts plans for small generated matrices under AddressSanitizer + UBSan and
prints every scalar and a hash of every array as it would be uploaded.  The expected lines were
recorded from the builders as they stood inside operator.c, before the unit existed."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")


def _run_dump(tmp_path_factory, defines, args):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/spmm_plan_dump.c")
    tmp = tmp_path_factory.mktemp("spmm_plan")
    exe, unit = str(tmp / "spmm_plan_dump"), str(tmp / "spmm_plan.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + defines + ["-c", os.path.join(CSRC, "spmm_plan.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "spmm_plan_dump.c"), unit, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or plan failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout.splitlines()


@pytest.fixture(scope="module")
def dump_lines(tmp_path_factory):
    return _run_dump(tmp_path_factory, [], [])


def test_plans_match_the_recorded_digests(dump_lines):
    with open(os.path.join(ROOT, "tests", "golden", "spmm_plan_digests.json")) as f:
        want = json.load(f)["lines"]
    assert len(dump_lines) == len(want)
    for got, ref in zip(dump_lines, want):
        assert got == ref


def test_cases_reach_every_plan_and_branch(dump_lines):
    """The recorded set is only worth something while it still holds every kind of plan."""
    def fields(line):
        head, rest = line.split(":", 1)
        kv = dict(x.split("=", 1) for x in rest.split())
        return head, {k: int(v) for k, v in kv.items() if k in
                      ("nslices", "nblk", "n_interior", "staged", "runs", "runs_cols", "win_cap")}
    plans = [fields(l) for l in dump_lines]
    kinds = {(p["staged"], p["runs"]) for _, p in plans}
    assert kinds == {(0, 0), (1, 0), (1, 1)}
    assert any(h.endswith("ts=16 cus=1 staged_switch=-1 runs_switch=1") and p["runs_cols"] == 8 for h, p in plans)
    assert any(p["staged"] and p["nblk"] < p["nslices"] for _, p in plans)        # blocks of several slices
    assert any(p["staged"] and p["nblk"] == p["nslices"] for _, p in plans)       # one-slice blocks
    assert all(not p["staged"] for h, p in plans if h.startswith("random4096"))   # a slice overflows: window plan
    # at one CU a block starts with three or four slices: more blocks than that means blocks were halved
    assert all(p["staged"] and p["nblk"] > (p["nslices"] + 2) // 3 for h, p in plans if h.startswith("random2048"))
    for kind in kinds:                                                            # halo-reading blocks come last
        assert any((p["staged"], p["runs"]) == kind and 0 < p["n_interior"] < p["nblk"] for _, p in plans)


def test_every_failed_allocation_is_reported_and_released(tmp_path_factory):
    """Each allocation of a build fails in turn (malloc, calloc, realloc, posix_memalign of the unit are
    routed through the program): the build answers -1 with an empty plan, and ASan / LeakSanitizer see
    no leak, no double free and no use of a block that a failed realloc left behind."""
    wrap = ["-D%s=t_%s" % (f, f) for f in ("malloc", "calloc", "realloc", "posix_memalign")]
    lines = _run_dump(tmp_path_factory, wrap, ["fail-allocs"])
    assert lines and all(l.split(": ")[1].startswith("every failed allocation handled") for l in lines)
    assert {l.rsplit(", ", 1)[1] for l in lines} == {"staged=0 runs=0", "staged=1 runs=0", "staged=1 runs=1"}
