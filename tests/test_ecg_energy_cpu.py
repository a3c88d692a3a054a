"""The host unit of the energy-norm error estimate (prealps_amd/csrc/ecg_energy.c) is arithmetic on a history of
drops: a stand-alone program (tests/c/ecg_energy_check.c) links it alone, is compiled with AddressSanitizer + UBSan and
run as a program, one mode per test.  The program holds the checks: the suffix sums against long double, the window
rule on hand-made sequences (geometric decay against the model bound, a plateau, one small drop between large ones,
drops below eps times the total, which a difference of prefix sums would turn into 0), the refusals, NaN, and what a
solve reports at its end."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/ecg_energy_check.c")
    tmp = tmp_path_factory.mktemp("ecg_energy")
    out, unit = str(tmp / "ecg_energy_check"), str(tmp / "ecg_energy.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "ecg_energy.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "ecg_energy_check.c"), unit, "-o", out, "-lm"])
    return out


@pytest.mark.parametrize("mode", ["sums", "rule", "small", "refusals", "nan", "report"])
def test_the_tracker_under_the_sanitizers(exe, mode):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().splitlines()[-1] == "ok"


def test_an_unknown_mode_is_no_success(exe):
    run = subprocess.run([exe, "nothing"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert run.returncode == 2
