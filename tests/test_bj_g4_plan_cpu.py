"""The launch planner of the band block solve (prealps_amd/csrc/bj_g4_plan.c: pa_bj_g4_plan): tile count, column sets,
DQ, occupancy hint, ring depth, wavefronts per workgroup, LDS bytes, grid, the Gram by-product and which of the three
chains of bj_g4.hip runs (plain, pipelined, PAIR).  tests/c/bj_g4_plan_check.c, a stand-alone program built with
AddressSanitizer + UBSan together with bj_g4_plan.c alone, plans every query of a grid that has both sides of every
dispatch edge; the plans are compared with a numpy restatement of the rules and checked on their own for what the
kernel needs whatever the rules say: the LDS it is given holds its ring, a chunk fits its buffer, the wait counter is
not overrun, the grid covers the work."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")

QF = ["count", "wmax", "bmax", "xs", "ncol", "bits", "gram", "cus", "ring_env", "pair_mode", "pair_intact", "have_tasks",
      "ntasks", "paired"]
PF = ["rc", "why", "kind", "nt", "nc", "dq", "occ", "gp", "bits", "ring", "waves", "per_wave", "lds", "blocks", "last_ring",
      "last_bits", "last_pipelined", "last_paired"]
PLAIN, PIPE, PAIR = 0, 1, 2
LDS_CU = 160 * 1024

BMAX = [1, 192, 193, 224, 225, 256, 257]
WMAX = [0, 16, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113]
PANEL = [(1, 4), (1, 8), (3, 4), (3, 8), (4, 4), (4, 8), (5, 8), (8, 8), (9, 16)]      # (ncol, xs): xs = ncol rounded up, and 8
BITS = [32, 64, 0]
RING = [0, 2, 4, 8, 3]
CUS = [0, 256]
COUNT = [1, 2047, 2048]
MODE = [-1, 0, 1]
INTACT = [0, 1]


def _product(*axes):
    """rows = the product of the axes; an axis is a 1-d or a 2-d array (several columns that move together)"""
    axes = [np.asarray(a, np.int32).reshape(len(a), -1) for a in axes]
    idx = np.meshgrid(*[np.arange(len(a), dtype=np.int16) for a in axes], indexing="ij")
    return np.concatenate([a[i.ravel()] for a, i in zip(axes, idx)], axis=1)


def grid():
    """int32 [n, 14] in the order of QF"""
    # (count, have_tasks, ntasks, paired): the pairs of a list of `count` blocks
    work = []
    for count in COUNT:
        for paired in sorted({0, 2, max(count // 2 - 1, 0), count // 2, count}):
            work.append((count, 1, max(count - paired // 2, 1), paired))
    main = _product(BMAX, WMAX, PANEL, BITS, RING, CUS, MODE, INTACT, work, [1])
    cols = ["bmax", "wmax", "ncol", "xs", "bits", "ring_env", "cus", "pair_mode", "pair_intact", "count", "have_tasks",
            "ntasks", "paired", "gram"]
    # the same without a Gram request, and without pair tasks at all (the pair fields at rest)
    rest = _product(BMAX, WMAX, PANEL, BITS, RING, CUS, [-1], [1], [(c, 1, (c + 1) // 2, c - c % 2) for c in COUNT], [0])
    none = _product(BMAX, WMAX, PANEL, BITS, RING, CUS, [-1, 1], [1], [(c, 0, 0, 0) for c in COUNT], [1])
    q = np.concatenate([main, rest, none])
    return np.ascontiguousarray(q[:, [cols.index(f) for f in QF]])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/bj_g4_plan_check.c")
    tmp = tmp_path_factory.mktemp("bj_g4_plan")
    exe, unit = str(tmp / "bj_g4_plan_check"), str(tmp / "bj_g4_plan.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "bj_g4_plan.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "bj_g4_plan_check.c"), unit, "-o", exe])
    return exe


def run_plans(exe, tmp, q):
    """the plans of the queries q: ({field: int64 array}, [reason texts])"""
    src, dst, txt = (os.path.join(str(tmp), n) for n in ("queries.bin", "plans.bin", "reasons.txt"))
    np.ascontiguousarray(q, np.int32).tofile(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, src, dst, txt], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    p = np.fromfile(dst, np.int32).reshape(-1, len(PF)).astype(np.int64)
    assert len(p) == len(q)
    with open(txt) as f:
        why = f.read().split("\n")[:-1]
    return {f: p[:, i] for i, f in enumerate(PF)}, why


@pytest.fixture(scope="module")
def planned(exe, tmp_path_factory):
    q = grid()
    p, why = run_plans(exe, tmp_path_factory.mktemp("bj_g4_plans"), q)
    return {f: q[:, i].astype(np.int64) for i, f in enumerate(QF)}, p, why


def restate(q):
    """the rules, in numpy: ({field: expected}, refused) -- the fields of a refused query mean nothing"""
    simds = 4 * np.where(q["cus"] > 0, q["cus"], 256)
    fp64 = q["bits"] == 64
    possible = ((q["have_tasks"] != 0) & (q["paired"] >= 2) & (q["pair_mode"] != 0) & (q["pair_intact"] != 0) & fp64
                & (q["xs"] <= 4) & (q["ncol"] <= 4) & (q["wmax"] <= 80))
    default = (q["bmax"] <= 192) & (q["wmax"] <= 48) & (q["count"] >= 2 * simds) & (2 * q["paired"] >= q["count"])
    pair = possible & ((q["pair_mode"] == 1) | default)
    nt = np.where(q["bmax"] > 224, 16, np.where(q["bmax"] > 192, 14, 12))
    nc = np.where(pair | (q["ncol"] > 4), 2, 1)
    dq = np.maximum(3, ((q["wmax"] + 15) >> 4) + 1)
    refused = (~np.isin(q["bits"], [32, 64])) | (q["bmax"] > 256) | (q["ncol"] > 8) | (dq > np.where(nc == 1, 8, 6))
    gram = (q["gram"] != 0) & (q["xs"] == 4) & (q["ncol"] == 4)
    # every launch but PAIR
    cbuf = (q["bits"] // 8 * (q["wmax"] + 4) + 127) & ~127
    nld = cbuf >> 7
    ring = np.where(np.isin(q["ring_env"], [2, 4, 8]), q["ring_env"], np.where(q["count"] < 2 * simds, 8, 2))
    for _ in range(2):
        ring = np.where((ring > 2) & (((ring - 1) * nld > 15) | (ring * cbuf * 8 > 40 * 1024)), ring >> 1, ring)
    waves = np.minimum(4, LDS_CU // np.maximum(ring * cbuf * 8, 1))
    refused |= ~pair & (waves < 1)
    pipe = ~pair & fp64 & (nc == 1) & (nt == 12) & (dq <= 5) & (ring >= 4)
    e = {"nt": nt, "nc": nc, "dq": dq, "bits": q["bits"]}
    e["kind"] = np.where(pair, PAIR, np.where(pipe, PIPE, PLAIN))
    e["occ"] = np.where(pipe, 1, np.where(nc == 2, 3, np.where((nt == 12) & (dq <= 5), 5, 4)))
    e["gp"] = (gram & (pair | (nc == 1))).astype(np.int64)
    e["ring"] = np.where(pair, 2, np.where(pipe, 4, ring))
    e["waves"] = np.where(pair, 4, np.where(pipe, 1, waves))
    e["per_wave"] = np.where(pair, 2 * dq * 128, np.where(pipe, 5 * dq * 128, ring * cbuf))
    e["lds"] = e["waves"] * e["per_wave"] * 8
    work = np.where(pair, q["ntasks"], q["count"])
    e["blocks"] = (work + e["waves"] - 1) // np.maximum(e["waves"], 1)
    e["last_ring"], e["last_bits"] = e["ring"], np.where(pair, 64, q["bits"])
    e["last_pipelined"], e["last_paired"] = pipe.astype(np.int64), pair.astype(np.int64)
    return e, refused


def test_every_plan_is_what_the_rules_say(planned):
    q, p, _ = planned
    e, refused = restate(q)
    assert np.array_equal(p["rc"], refused.astype(np.int64))
    ok = ~refused
    for f in e:
        bad = np.nonzero(ok & (p[f] != e[f]))[0]
        assert bad.size == 0, (f, {k: int(q[k][bad[0]]) for k in QF}, int(p[f][bad[0]]), int(e[f][bad[0]]))


def test_every_plan_gives_the_kernel_what_it_needs(planned):
    q, p, _ = planned
    ok = p["rc"] == 0
    q = {f: a[ok] for f, a in q.items()}
    p = {f: a[ok] for f, a in p.items()}
    plain, pipe, pair = p["kind"] == PLAIN, p["kind"] == PIPE, p["kind"] == PAIR
    assert np.all(plain | pipe | pair)
    assert np.all(np.isin(p["bits"], [32, 64])) and np.array_equal(p["bits"], q["bits"])
    # the template arguments cover the class: rows in nt tiles, the band in dq tiles, the columns in nc sets
    assert np.all(np.isin(p["nt"], [12, 14, 16])) and np.all(q["bmax"] <= 16 * p["nt"])
    assert np.all(q["wmax"] + 15 < 16 * p["dq"]) and np.all(p["dq"] >= 3)
    assert np.all(p["dq"] <= np.where(p["nc"] == 1, 8, 6))
    assert np.all(np.isin(p["nc"], [1, 2])) and np.all(q["ncol"] <= np.where(pair, 4, 4 * p["nc"]))
    # the LDS: what the launch asks for is what the wavefronts use, and a workgroup can have it
    assert np.array_equal(p["lds"], p["waves"] * p["per_wave"] * 8)
    assert np.all(p["lds"] <= LDS_CU) and np.all(p["waves"] >= 1) and np.all(p["waves"] <= 4)
    # a chunk (two groups of wmax + 4 rows x 4 pivots) fits its ring buffer; the pipelined chain has a spare buffer
    chunk = p["bits"] // 8 * (q["wmax"] + 4)
    assert np.all(chunk <= p["per_wave"] // (p["ring"] + pipe))
    assert np.all(np.isin(p["ring"], [2, 4, 8]))
    # the plain chain waits by a count of LDS-DMA pieces (1 KiB) that the hardware counter (vmcnt < 64, the kernel's
    # switch up to 15) must hold: ring - 1 chunks in flight
    nld = (chunk + 127) >> 7
    assert np.all(((p["ring"] - 1) * nld)[plain] <= 15)
    # PAIR: ring 2 (the wait counts of its Gram rows are written for that depth), fp64 records, panels of <= 4 columns
    assert np.all(p["ring"][pair] == 2) and np.all(p["bits"][pair] == 64) and np.all(p["nc"][pair] == 2)
    assert np.all(q["xs"][pair] <= 4) and np.all(q["have_tasks"][pair] == 1) and np.all(q["pair_mode"][pair] != 0)
    assert np.all(q["pair_intact"][pair] == 1) and np.all(p["per_wave"][pair] == 2 * p["dq"][pair] * 128)
    # PIPE: only the kernels that exist -- fp64 records, one column set, 12 tiles, DQ <= 5 -- with the compile-time ring
    assert np.all((p["bits"] == 64)[pipe]) and np.all((p["nc"] == 1)[pipe]) and np.all((p["nt"] == 12)[pipe])
    assert np.all((p["dq"] <= 5)[pipe]) and np.all(p["ring"][pipe] == 4) and np.all(p["waves"][pipe] == 1)
    assert np.all(p["per_wave"][pipe] == 5 * p["dq"][pipe] * 128) and np.all(q["ring_env"][pipe] != 2)
    # the grid covers the work, without an empty workgroup
    work = np.where(pair, q["ntasks"], q["count"])
    assert np.all(p["blocks"] * p["waves"] >= work) and np.all((p["blocks"] - 1) * p["waves"] < work)
    # the Gram by-product: an 8 x 4 block of a 4-column panel, when asked for, on kernels that have it
    gp = p["gp"] == 1
    assert np.all(np.isin(p["gp"], [0, 1])) and gp.any()
    assert np.all((q["xs"] == 4)[gp]) and np.all((q["ncol"] == 4)[gp]) and np.all((q["gram"] == 1)[gp])
    assert np.all(((p["nc"] == 1) | pair)[gp])
    # the occupancy hint is one the kernels are compiled with
    assert np.all(p["occ"] == np.where(pipe, 1, np.where(p["nc"] == 2, 3, np.where((p["nt"] == 12) & (p["dq"] <= 5), 5, 4))))
    # what the library reports about the launch
    assert np.array_equal(p["last_ring"], p["ring"]) and np.array_equal(p["last_bits"], p["bits"])
    assert np.array_equal(p["last_pipelined"], pipe.astype(np.int64)) and np.array_equal(p["last_paired"], pair.astype(np.int64))


def test_every_refusal_names_the_offending_value(planned):
    q, p, why = planned
    no = p["rc"] == 1
    assert no.any() and np.all(np.isin(p["rc"], [0, 1]))
    assert all(why[i] == "" for i in np.unique(p["why"][~no])), "a plan that was made carries a reason"
    # the distinct (reason, bits, rows, columns, band) of the refused queries, through one packed key
    key = np.unique(((((p["why"] << 7 | q["bits"]) << 9 | q["bmax"]) << 4 | q["ncol"]) << 7 | q["wmax"])[no])
    keys = np.stack([key >> 27, key >> 20 & 127, key >> 11 & 511, key >> 7 & 15, key & 127], axis=1)
    seen = set()
    for w, bits, bmax, ncol, wmax in keys.tolist():
        d = max(3, ((wmax + 15) >> 4) + 1)
        text = why[w]
        assert text.strip(), "a refusal without a reason"
        numbers = set(int(x) for x in re.findall(r"-?\d+", text))
        # the values of this query that a limit excludes, or may (a band above 80: on two column sets), with the limit
        offending = [(v, lim, name) for v, lim, name, off in
                     ((bits, {64}, "bits", bits not in (32, 64)), (bmax, {256}, "rows", bmax > 256), (ncol, {8}, "columns", ncol > 8),
                      (wmax, {80, 112} if d > 8 else {80}, "band", d > 6)) if off]
        named = [(v, lim, name) for v, lim, name in offending if v in numbers and lim & numbers]
        assert named, (text, offending)
        seen.update(name for _, _, name in named)
    assert seen == {"bits", "rows", "columns", "band"}


def _count(p, sel, kind, nt=None, dq=None):
    m = sel & (p["rc"] == 0) & (p["kind"] == kind)
    if nt is not None:
        m &= p["nt"] == nt
    if dq is not None:
        m &= p["dq"] == dq
    return int(np.count_nonzero(m))


def test_the_grid_has_both_sides_of_every_edge(planned):
    q, p, _ = planned
    ok = p["rc"] == 0
    # plans per (kind, nt, dq): every kernel family is reached, and nothing beyond
    key, n = np.unique((p["kind"] * 100 + p["nt"])[ok] * 100 + p["dq"][ok], return_counts=True)
    plans = {(int(k) // 10000, int(k) // 100 % 100, int(k) % 100): int(c) for k, c in zip(key, n)}
    want = {(PLAIN, nt, dq) for nt in (12, 14, 16) for dq in range(3, 9)} | {(PIPE, 12, dq) for dq in (3, 4, 5)} | \
           {(PAIR, nt, dq) for nt in (12, 14, 16) for dq in range(3, 7)}
    assert set(plans) == want and min(plans.values()) > 0, plans
    # tiles: 192 | 193, 224 | 225, 256 | 257 rows
    for bmax, nt in ((1, 12), (192, 12), (193, 14), (224, 14), (225, 16), (256, 16)):
        assert np.all(p["nt"][ok & (q["bmax"] == bmax)] == nt) and np.any(ok & (q["bmax"] == bmax))
    assert not np.any(ok & (q["bmax"] == 257)) and np.any(q["bmax"] == 257)
    # DQ: the last band of each ring-buffer size and the first of the next; 112 | 113 on one column set, 80 | 81 on two
    fine = np.isin(q["bits"], [32, 64]) & (q["bmax"] <= 256) & (q["ncol"] <= 8)          # nothing but the band to refuse
    for wmax, dq in zip(WMAX, (3, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9)):
        m = fine & (q["wmax"] == wmax)
        assert np.any(ok & m) == (dq <= 8) and np.all(p["dq"][ok & m] == dq) and np.any(~ok & m) == (dq > 6)
        assert np.any(ok & m & (p["nc"] == 2)) == (dq <= 6) and np.any(~ok & m & (q["ncol"] > 4)) == (dq > 6)
        assert np.any(~ok & m & (q["ncol"] <= 4)) == (dq > 8)
    # column sets: 4 | 5 columns, 8 | 9
    assert np.all(p["nc"][ok & (q["ncol"] == 5)] == 2) and np.any(ok & (q["ncol"] == 4) & (p["nc"] == 1))
    assert np.any(ok & (q["ncol"] == 8)) and not np.any(ok & (q["ncol"] == 9))
    # record bits
    assert np.any(ok & (q["bits"] == 32)) and np.any(ok & (q["bits"] == 64)) and not np.any(ok & (q["bits"] == 0))
    # ring: 2047 | 2048 blocks on 256 compute units, the environment's 2 / 4 / 8 and a value it ignores; every depth
    auto = ok & (p["kind"] != PAIR) & np.isin(q["ring_env"], [0, 3]) & (q["wmax"] == 0) & (q["bits"] == 32)
    assert np.all(p["ring"][auto & (q["count"] == 2047)] == 8) and np.all(p["ring"][auto & (q["count"] == 2048)] == 2)
    for ring in (2, 4, 8):
        assert _count(p, p["ring"] == ring, PLAIN) > 0
        assert _count(p, (q["ring_env"] == ring) & (p["ring"] < ring), PLAIN) > 0 or ring == 2      # the halving
    assert _count(p, q["ring_env"] == 2, PIPE) == 0 and _count(p, q["ring_env"] == 4, PIPE) > 0
    assert _count(p, (q["ring_env"] == 0) & (q["count"] == 2047), PIPE) > 0
    assert _count(p, (q["ring_env"] == 0) & (q["count"] == 2048), PIPE) == 0
    # PAIR, the default rule: each condition on both sides, the others held where they allow it
    base = (q["pair_mode"] == -1) & (q["pair_intact"] == 1) & (q["bits"] == 64) & (q["xs"] == 4) & (q["count"] == 2048) & \
           (q["paired"] == 2048) & (q["bmax"] == 192) & (q["wmax"] == 48) & (q["have_tasks"] == 1)
    assert _count(p, base, PAIR) > 0 and _count(p, base, PLAIN) + _count(p, base, PIPE) == 0

    def flipped(**kw):
        m = (q["pair_mode"] == -1) & (q["have_tasks"] == 1)
        for f, v in dict(dict(pair_intact=1, bits=64, xs=4, count=2048, paired=2048, bmax=192, wmax=48), **kw).items():
            m &= q[f] == v
        return m
    for kw in (dict(wmax=49), dict(bmax=193), dict(count=2047, paired=2047), dict(paired=1023), dict(pair_intact=0),
               dict(bits=32), dict(xs=8), dict(paired=0)):
        assert np.any(flipped(**kw)) and _count(p, flipped(**kw), PAIR) == 0, kw
    assert _count(p, flipped(paired=1024), PAIR) > 0
    # mode 1 pairs wherever it is possible (bands up to 80 | 81, any rows, few blocks), mode 0 never
    forced = (q["pair_mode"] == 1) & (q["pair_intact"] == 1) & (q["bits"] == 64) & (q["xs"] == 4) & (q["paired"] >= 2) & \
             (q["have_tasks"] == 1) & (q["bmax"] <= 256)
    assert np.all(p["kind"][ok & forced & (q["wmax"] <= 80)] == PAIR) and _count(p, forced & (q["wmax"] == 80) & (q["bmax"] == 256), PAIR) > 0
    assert _count(p, forced & (q["wmax"] == 81), PAIR) == 0 and _count(p, forced & (q["wmax"] == 81), PLAIN) > 0
    assert _count(p, q["pair_mode"] == 0, PAIR) == 0 and _count(p, q["have_tasks"] == 0, PAIR) == 0
    # the Gram by-product: on every chain, and not without a request or off the 4-column panel
    for kind in (PLAIN, PIPE, PAIR):
        assert _count(p, p["gp"] == 1, kind) > 0 and _count(p, p["gp"] == 0, kind) > 0
    assert not np.any(ok & (p["gp"] == 1) & (q["gram"] == 0)) and np.any(ok & (q["gram"] == 0) & (q["xs"] == 4) & (q["ncol"] == 4))
