"""The band map behind preAlps_BlockJacobiUpdateValues (prealps_amd/csrc/bj_band_map.c): which panel entry every
entry of an assembled band is.  tests/c/bj_band_map_check.c, a stand-alone program built with AddressSanitizer +
UBSan like the value-map check of test_value_map_cpu.py, holds it against a direct assembly of every band from the
permuted dense diagonal block: the same bits for two value arrays, every in-block lower-triangle entry used exactly
once, unique destinations inside their block, nothing from sparse-factored blocks."""
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
        pytest.fail("gcc is needed to build tests/c/bj_band_map_check.c")
    tmp = tmp_path_factory.mktemp("bj_band_map")
    exe, unit = str(tmp / "bj_band_map_check"), str(tmp / "bj_band_map.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "bj_band_map.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "bj_band_map_check.c"), unit, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or map failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout.splitlines()


def _fields(line):
    head, rest = line.split(": ", 1)
    return head, {k: int(v) for k, v in (x.split("=", 1) for x in rest.split())}


def test_the_map_is_the_assembly_of_every_band(check_lines):
    """The program exits non-zero on any violation (the fixture asserts that); here: the runs still cover what they
    are meant to cover."""
    cases = [_fields(l) for l in check_lines]
    assert len(cases) == 5 * 4 + 3
    for panel in ("poisson12", "nodes8", "random2048", "poisson12_shard", "nodes8_shard", "poisson12_doubled"):
        assert any(h.startswith(panel + " ") for h, _ in cases), panel
    assert all(f["entries"] > 0 and f["chunks"] > 0 for _, f in cases)
    # both layouts inside one run, on a whole panel and on a shard
    assert any(f["rows"] > 0 and f["diag"] > 0 for h, f in cases if h.startswith("nodes8 "))
    assert any(f["rows"] > 0 and f["diag"] > 0 for h, f in cases if "_shard " in h)
    # sparse-factored blocks in the runs that flag them, and only there
    assert all((f["nd"] > 0) == ("nd_every=3" in h) for h, f in cases)
    # a small chunk size cuts a block into several chunks
    assert any("chunk=100" in h and f["chunks"] > 2 * f["blocks"] for h, f in cases)


def test_a_doubled_column_keeps_one_entry(check_lines):
    cases = [_fields(l) for l in check_lines]
    assert all((f["doubled"] > 0) == h.startswith("poisson12_doubled ") for h, f in cases if "shift=0" in h)
    plain = [f for h, f in cases if h.startswith("poisson12 shift=0 nd_every=0 wmax=200")]
    doubled = [f for h, f in cases if h.startswith("poisson12_doubled shift=0")]
    assert len(plain) == 1 and len(doubled) == 1 and plain[0]["entries"] == doubled[0]["entries"]
