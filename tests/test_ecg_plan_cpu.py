"""The pool layout and the switch decisions of an ECG solver (prealps_amd/csrc/ecg_plan.c) are plain host arithmetic:
a stand-alone program (tests/c/ecg_plan_check.c) links the unit alone, is compiled with AddressSanitizer + UBSan and
run as a program.  It prints what the unit answers for every case; the list of regions and the rules are restated here,
independently of the C code."""
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
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/ecg_plan_check.c")
    tmp = tmp_path_factory.mktemp("ecg_plan")
    out, unit = str(tmp / "ecg_plan_check"), str(tmp / "ecg_plan.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "ecg_plan.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "ecg_plan_check.c"), unit, "-o", out])
    return out


def rows(exe, mode):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stderr[-4000:]
    return [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]


def test_the_unit_includes_its_own_header_and_stddef_only():
    src = open(os.path.join(CSRC, "ecg_plan.c")).read() + open(os.path.join(CSRC, "ecg_plan.h")).read()
    includes = sorted(set(line.split()[1] for line in src.splitlines() if line.startswith("#include")))
    assert includes == ['"ecg_plan.h"', "<stddef.h>"]
    assert "getenv" not in src


REGIONS = ["V0", "V1", "AV0", "AV1", "Z", "R", "X", "F", "q", "res2", "uu", "partials", "rtr_part", "spmm_parts",
           "bj_parts", "grp", "sys_part"]


def expected_layout(m, T, ts, alg, spmm_cap, bj_cap, G, S):
    """The regions in order as (name, size or None when absent)."""
    panel = max(m, 1) * ts
    nv = 1 if alg == ORTHOMIN else 2
    return [("V0", panel), ("V1", panel if nv == 2 else None), ("AV0", panel), ("AV1", panel if nv == 2 else None),
            ("Z", panel), ("R", panel), ("X", panel), ("F", 5 * T * T), ("q", 2 * T * T), ("res2", 24), ("uu", 2 * T * T),
            ("partials", G * 2 * ts * ts), ("rtr_part", G * ts),
            ("spmm_parts", (spmm_cap + S) * 32 if spmm_cap > 0 else None),
            ("bj_parts", (bj_cap + S) * 32 if bj_cap > 0 else None), ("grp", 48), ("sys_part", G * ts)]


def test_pool_layout(exe):
    got = rows(exe, "layout")
    want_inputs = set(itertools.product([0, 1, 5, 1000], [(1, 2), (2, 2), (3, 4), (4, 4), (8, 8), (12, 16), (16, 16)],
                                        [ORTHOMIN, ORTHODIR, ORTHODIR_FUSED], [0, 7], [0, 9]))
    seen, Gs, Ss = set(), set(), set()
    for row in got:
        m, T, ts, alg, spmm_cap, bj_cap, G, S = row[:8]
        o = dict(zip(["V0", "V1", "AV0", "AV1", "Z", "R", "X", "F", "alpha", "beta", "mu", "rtr", "q", "res2", "uu",
                      "partials", "rtr_part", "spmm_parts", "bj_parts", "grp", "sys_part", "pool_doubles"], row[8:]))
        assert len(row) == 8 + 22
        seen.add((m, (T, ts), alg, spmm_cap, bj_cap)); Gs.add(G); Ss.add(S)
        at, spans = 0, []
        for name, size in expected_layout(m, T, ts, alg, spmm_cap, bj_cap, G, S):
            if size is None:
                assert o[name] == -1, (row, name)
                continue
            assert o[name] == at, (row, name)                  # every offset, region by region
            spans.append((o[name], o[name] + size))
            at += size
        assert o["pool_doubles"] == at                          # the regions end at pool_doubles ...
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):        # ... ascending and disjoint (adjacent: no gap either)
            assert a0 < a1 == b0 < b1
        assert spans[0][0] == 0 and spans[-1][1] == o["pool_doubles"]
        # the blocks inside F
        assert (o["alpha"], o["beta"], o["mu"], o["rtr"]) == (o["F"], o["F"] + T * T, o["F"] + 3 * T * T, o["F"] + 4 * T * T)
        # the sum the allocation used to state: (2 nv + 3) panels + small + parts
        panel, nv = max(m, 1) * ts, (1 if alg == ORTHOMIN else 2)
        small = 5 * T * T + 2 * T * T + 24 + 2 * T * T
        parts = G * (2 * ts * ts + ts) + ((spmm_cap + S) * 32 if spmm_cap else 0) + ((bj_cap + S) * 32 if bj_cap else 0) + 48 + G * ts
        assert o["pool_doubles"] == (2 * nv + 3) * panel + small + parts
        assert (o["V1"] == -1) == (o["AV1"] == -1) == (alg == ORTHOMIN)
        assert (o["spmm_parts"] == -1) == (spmm_cap == 0) and (o["bj_parts"] == -1) == (bj_cap == 0)
    assert seen == want_inputs and len(Gs) == 2 and len(Ss) == 2
    assert len(got) == len(want_inputs) * 4


def expected_switches(alg, bs_red, enlFac, nrhs, guess, metric, world, loopback, timing, fuse, lazy_norm_sw, lazy_stop_sw,
                      graphs, poll_sw):
    rotate = bs_red == NO_BS_RED
    lazy_norm = bool(fuse and alg == ORTHODIR and lazy_norm_sw)
    lazy_stop = bool(fuse and bs_red == NO_BS_RED and alg != ORTHODIR_FUSED and enlFac >= 2 and lazy_stop_sw)
    request = 0 if (nrhs > 1 or guess or metric) else graphs
    use_graphs = bool(request and (world == 1 or loopback or request == 2) and rotate and fuse and alg != ORTHODIR_FUSED
                      and not timing)
    if use_graphs:
        lazy_stop = False
    poll = bool((poll_sw != 0 if poll_sw >= 0 else world > 1) and not use_graphs)
    if nrhs > 1 or guess or metric:
        poll = False
    ride = nrhs > 1 and not metric and world > 1
    return tuple(int(v) for v in (rotate, fuse, lazy_norm, lazy_stop, use_graphs, poll, ride))


def test_switch_table(exe):
    got = rows(exe, "switches")
    want_inputs = set(itertools.product([ORTHOMIN, ORTHODIR, ORTHODIR_FUSED], [ADAPT_BS, NO_BS_RED], [1, 2, 4, 8], [1, 2],
                                        [0, 1], [0, 1], [(1, 0), (1, 1), (8, 0)], [0, 1], [0, 1], [0, 1], [0, 1], [0, 1, 2],
                                        [-1, 0, 1]))
    assert len(got) == len(want_inputs) == 82944
    seen = set()
    for row in got:
        assert len(row) == 21
        i = row[:14]
        seen.add(i[:6] + ((i[6], i[7]),) + i[8:])
        assert row[14:] == expected_switches(*i), row
    assert seen == want_inputs
