"""The dispatch planner of the band block solve (prealps_amd/csrc/bj_band_plan.c: pa_bj_band_plan): which of k_bj_g4,
k_bj_mfma, k_bj_apply_pairs, k_bj_apply and k_bj_wide serves a bandwidth class at a panel width, the template arguments
of the instance and the numbers of its launch.  tests/c/bj_band_plan_check.c, a stand-alone program built with
AddressSanitizer + UBSan together with bj_band_plan.c alone, plans every query of a grid that has both sides of every
dispatch edge; the plans are compared with a numpy restatement of the rules and checked on their own for what the
kernels need whatever the rules say (read from bj_band.hip): a chunk of the widest record fits its buffer, the LDS the
launch asks for is what its wavefronts use and a workgroup can have it, the tiles cover the band, the grid covers the
work.  Every refusal names its number, every instance bj_band.hip compiles is reached and nothing else is, no class the
layout can make is refused for lack of LDS, and the family labels of tests/test_gpu_band_blocks.py (_family) are what
the planner picks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")

QF = ["ts", "R", "wmax", "count", "have_g4", "have_pairs", "g4_wide", "mfma", "cus"]
PF = ["rc", "why", "family", "ts", "xs", "r", "ch", "tiles", "cap", "waves", "per_wave", "nbuf", "lds", "blocks", "threads"]
G4, MFMA, PAIRS, APPLY, WIDE = range(5)
LDS_CU = 160 * 1024
MAX_R = 8                   # PA_BJ_MAX_R

TS = [1, 2, 3, 4, 8, 16, 32]
RS = [-4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
WMAX = [0, 47, 48, 49, 80, 81, 112, 113,                      # the tiles of k_bj_mfma, the 8-column limit of k_bj_g4
        127, 128, 129, 191, 192, 193, 447, 448, 449,          # the class edges of R
        704, 705, 960, 961, 1472, 1473, 1984, 1985, 3008, 3009, 4032, 4033,   # windows of 12 | 13 and 16 | 17 wavefronts at 1 / 2 / 4 register sets
        319, 320, 415, 416, 639, 640, 1279, 1280,             # plain records: 4 | 3 | 2 | 1 | no wavefronts per workgroup by the LDS
        1276, 1277]                                           # paired records: the last that fits | the first that does not
COUNT = [1, 1023, 1024, 5670]                                 # 4 * 256 compute units - 1 | 4 * 256
CUS = [0, 256]


def window(w):
    """pa_bj_wide_window (pa_device.h)"""
    w = np.asarray(w, np.int64)
    return np.where(((w + 127) & ~63) <= 1024, (w + 127) & ~63, np.where(((w + 191) & ~127) <= 2048, (w + 191) & ~127, (w + 319) & ~255))


def _product(*axes):
    axes = [np.asarray(a, np.int32) for a in axes]
    idx = np.meshgrid(*[np.arange(len(a), dtype=np.int16) for a in axes], indexing="ij")
    return np.stack([a[i.ravel()] for a, i in zip(axes, idx)], axis=1)


def grid():
    """int32 [n, 9] in the order of QF"""
    return np.ascontiguousarray(_product(TS, RS, WMAX, COUNT, [0, 1], [0, 1], [0, 1], [0, 1, 2], CUS))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/bj_band_plan_check.c")
    tmp = tmp_path_factory.mktemp("bj_band_plan")
    exe, unit = str(tmp / "bj_band_plan_check"), str(tmp / "bj_band_plan.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "bj_band_plan.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "bj_band_plan_check.c"), unit, "-o", exe])
    return exe


def run_plans(exe, tmp, q):
    """the plans of the queries q: ({field: int64 array} of the queries, the same of the plans, [reason texts])"""
    src, dst, txt = (os.path.join(str(tmp), n) for n in ("queries.bin", "plans.bin", "reasons.txt"))
    np.ascontiguousarray(q, np.int32).tofile(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, src, dst, txt], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    p = np.fromfile(dst, np.int32).reshape(-1, len(PF)).astype(np.int64)
    assert len(p) == len(q)
    with open(txt) as f:
        why = f.read().split("\n")[:-1]
    return {f: np.asarray(q)[:, i].astype(np.int64) for i, f in enumerate(QF)}, {f: p[:, i] for i, f in enumerate(PF)}, why


@pytest.fixture(scope="module")
def planned(exe, tmp_path_factory):
    return run_plans(exe, tmp_path_factory.mktemp("bj_band_plans"), grid())


def restate(q):
    """the rules, in numpy: ({field: expected}, {refusal: mask}) -- the fields of a refused query mean nothing, and of a
    G4 plan only the family does"""
    ts, R, wmax = q["ts"], q["R"], q["wmax"]
    g4 = (q["have_g4"] != 0) & ((ts <= 4) | ((ts == 8) & (q["g4_wide"] != 0) & (wmax <= 80)))
    rest = ~g4
    no = {"stride": rest & ~np.isin(ts, [2, 4, 8, 16])}
    rest = rest & ~no["stride"]
    wide, Rw = rest & (R < 0), np.maximum(-R, 1)
    W = window(wmax)
    nw = (W + 64 * Rw - 1) // (64 * Rw)
    no["sets"] = wide & ~np.isin(Rw, [1, 2, 4])
    no["window"] = wide & ~no["sets"] & ((nw > 16) | (ts * Rw > 16))
    wide = wide & ~no["sets"] & ~no["window"]
    no["class"] = rest & (R >= 0) & ((R < 1) | (R > MAX_R))
    narrow = rest & (R >= 1) & (R <= MAX_R)
    mfma = narrow & (wmax <= 112) & (((ts >= 8) & (q["mfma"] == 1)) | (q["mfma"] == 2))
    pairs = narrow & ~mfma & (q["have_pairs"] != 0) & (ts <= 4) & np.isin(R, [2, 3])
    split = narrow & ~mfma & (ts == 4) & (q["count"] < 4 * np.where(q["cus"] > 0, q["cus"], 256))
    rec = np.where(pairs, wmax + 4, (wmax + 2) & ~1)
    per_wave = 2 * ((8 * rec + 127) & ~127)
    waves = np.minimum(4, LDS_CU // (per_wave * 8))
    no["lds"] = narrow & (waves < 1)
    e = {"family": np.where(g4, G4, np.where(wide, WIDE, np.where(mfma, MFMA, np.where(pairs, PAIRS, APPLY))))}
    e["ts"], e["xs"] = np.where(split, 2, ts), ts
    e["r"] = np.where(wide, Rw, R)
    e["ch"] = np.where(wide, 0, 8)
    e["tiles"] = np.where(mfma, np.where(wmax <= 48, 4, np.where(wmax <= 80, 6, 8)), 0)
    e["cap"] = np.where(wide, np.where(nw <= 12, 768, 1024), 0)
    e["waves"] = np.where(wide, nw, waves)
    e["per_wave"], e["nbuf"] = np.where(wide, 0, per_wave), np.where(wide, 0, 2)
    e["lds"] = e["waves"] * e["per_wave"] * 8
    units = np.where(mfma, q["count"], q["count"] * (e["xs"] // np.maximum(e["ts"], 1)))
    e["blocks"] = np.where(wide, q["count"], (units + e["waves"] - 1) // np.maximum(e["waves"], 1))
    e["threads"] = 64 * e["waves"]
    return e, no


def test_every_plan_is_what_the_rules_say(planned):
    q, p, _ = planned
    e, no = restate(q)
    refused = np.any(list(no.values()), axis=0)
    assert np.array_equal(p["rc"], refused.astype(np.int64))
    ok = ~refused
    assert np.array_equal(p["family"][ok], e["family"][ok])
    for f in e:
        bad = np.nonzero(ok & (p["family"] != G4) & (p[f] != e[f]))[0]
        assert bad.size == 0, (f, {k: int(q[k][bad[0]]) for k in QF}, int(p[f][bad[0]]), int(e[f][bad[0]]))
    g4 = ok & (p["family"] == G4)          # k_bj_g4 has its own planner: nothing but the family comes from this one
    assert g4.any() and all(not np.any(p[f][g4]) for f in PF if f not in ("rc", "why"))


def test_every_plan_gives_the_kernel_what_it_needs(planned):
    q, p, _ = planned
    ok = (p["rc"] == 0) & (p["family"] != G4)
    q = {f: a[ok] for f, a in q.items()}
    p = {f: a[ok] for f, a in p.items()}
    wide, mfma, pairs, apply_ = (p["family"] == f for f in (WIDE, MFMA, PAIRS, APPLY))
    chunked = ~wide
    assert np.all(wide | mfma | pairs | apply_) and all(m.any() for m in (wide, mfma, pairs, apply_))
    # an instance exists for the stride, and it solves whole panels: XS is the stride, TS divides it
    assert np.all(np.isin(q["ts"], [2, 4, 8, 16])) and np.array_equal(p["xs"], q["ts"]) and np.all(p["xs"] % p["ts"] == 0)
    # k_bj_apply / k_bj_apply_pairs / k_bj_mfma: a wavefront reads chunks of 8 records (bj_chunk, bj_chunk_pairs, the
    # `8 * wr` of k_bj_mfma) of the class's widest band into one of nbuf buffers and is given nbuf such buffers
    rec = np.where(pairs, q["wmax"] + 4, (q["wmax"] + 2) & ~1)
    assert np.all(p["ch"][chunked] == 8) and np.all(p["nbuf"][chunked] == 2)
    assert np.all((8 * rec * p["nbuf"] <= p["per_wave"])[chunked]) and np.all(p["per_wave"][chunked] % (p["nbuf"][chunked] * 128) == 0)
    # the LDS: what the launch asks for is what the wavefronts use, and a workgroup can have it
    assert np.array_equal(p["lds"], p["waves"] * p["per_wave"] * 8) and np.all(p["lds"] <= LDS_CU)
    assert np.all(p["waves"] >= 1) and np.array_equal(p["threads"], 64 * p["waves"])
    assert np.all(p["threads"][chunked] <= 256)                      # __launch_bounds__(256)
    # k_bj_mfma: no attribute is set for it, so at most 64 KiB; its tiles hold a band and its 16 pivots; bands up to 112
    assert np.all(p["lds"][mfma] <= 64 * 1024) and np.all((16 * p["tiles"] >= q["wmax"] + 16)[mfma])
    assert np.all(np.isin(p["tiles"][mfma], [4, 6, 8])) and np.all(q["wmax"][mfma] <= 112)
    assert np.array_equal(p["ts"][mfma], q["ts"][mfma])
    # the register recurrence holds bands up to 64 R - 64 ... which the class guarantees, not the planner: R is passed on
    assert np.array_equal(p["r"][chunked], q["R"][chunked]) and np.all((p["r"] >= 1)[chunked]) and np.all((p["r"] <= MAX_R)[chunked])
    # paired records: classes 2 and 3 at up to 4 columns, only where they exist
    assert np.all(np.isin(p["r"][pairs], [2, 3])) and np.all(q["ts"][pairs] <= 4) and np.all(q["have_pairs"][pairs] == 1)
    # one wavefront per block and column group (k_bj_mfma: per block), no empty workgroup
    units = np.where(mfma, q["count"], q["count"] * p["xs"] // p["ts"])
    assert np.all((p["waves"] * p["blocks"] >= units)[chunked]) and np.all(((p["blocks"] - 1) * p["waves"] < units)[chunked])
    # k_bj_wide: one workgroup per block; the window in flight across the wavefronts of R register sets, TS columns of
    # each per lane (TS * R <= 16 accumulators); the instance bounded for 768 threads only up to 12 wavefronts
    W = window(q["wmax"])
    assert np.array_equal(p["blocks"][wide], q["count"][wide]) and np.all(np.isin(p["r"][wide], [1, 2, 4]))
    assert np.all((64 * p["r"] * p["waves"] >= W)[wide]) and np.all((64 * p["r"] * (p["waves"] - 1) < W)[wide])
    assert np.all(p["waves"][wide] <= 16) and np.all((p["ts"] * p["r"] <= 16)[wide])
    assert np.all(np.isin(p["cap"][wide], [768, 1024])) and np.all((p["threads"] <= p["cap"])[wide])
    assert np.all((p["waves"] <= 12)[wide & (p["cap"] == 768)]) and np.all(p["lds"][wide] == 0)


# what bj_band.hip compiles: (family, TS, XS, R, tiles, thread cap)
INSTANCES = ({(APPLY, t, t, r, 0, 0) for t in (2, 4, 8, 16) for r in range(1, 9)} | {(APPLY, 2, 4, r, 0, 0) for r in range(1, 9)} |
             {(PAIRS, t, x, r, 0, 0) for t, x in ((2, 2), (4, 4), (2, 4)) for r in (2, 3)} |
             {(MFMA, t, t, 0, n, 0) for t in (2, 4, 8, 16) for n in (4, 6, 8)} |
             {(WIDE, t, t, r, 0, c) for t in (2, 4, 8, 16) for r in (1, 2, 4) if t * r <= 16 for c in (768, 1024)})


def test_the_instances_reached_are_the_instances_compiled(planned):
    _, p, _ = planned
    ok = (p["rc"] == 0) & (p["family"] != G4)
    r = np.where(p["family"] == MFMA, 0, p["r"])          # (k_bj_mfma has no R)
    got = np.unique(np.stack([p["family"], p["ts"], p["xs"], r, p["tiles"], p["cap"]], axis=1)[ok], axis=0)
    assert {tuple(int(x) for x in row) for row in got} == INSTANCES
    assert np.all(p["ch"][ok & (p["family"] != WIDE)] == 8)


def test_every_refusal_names_the_offending_value(planned):
    q, p, why = planned
    _, no = restate(q)
    refused = p["rc"] == 1
    assert np.all(np.isin(p["rc"], [0, 1])) and all(why[i] == "" for i in np.unique(p["why"][~refused]))
    for kind, mask in no.items():
        assert mask.any() and np.all(refused[mask]), kind
        rows = np.unique(np.stack([p["why"], q["ts"], q["R"], q["wmax"], q["have_pairs"]], axis=1)[mask], axis=0)
        for w, ts, R, wmax, have_pairs in rows.tolist():
            text = why[w]
            numbers = [int(x) for x in re.findall(r"-?\d+", text)]
            if kind == "stride":
                assert text == "unsupported panel stride %d" % ts
            elif kind == "sets":
                assert "register sets" in text and numbers == [-R, 1, 2, 4], text
            elif kind == "window":
                assert text == ("bandwidth %d is too wide for panel stride %d (window %d rows); use more subdomains"
                                % (wmax, ts, int(window(wmax)))), text
            elif kind == "class":
                assert "class" in text and numbers == [R, 1, MAX_R], text
            else:
                rec = wmax + 4 if have_pairs and ts <= 4 and R in (2, 3) else (wmax + 2) & ~1
                assert "LDS" in text and numbers == [2 * ((8 * rec + 127) & ~127) * 8, LDS_CU], text


def test_the_grid_has_both_sides_of_every_edge(planned):
    q, p, _ = planned
    ok = p["rc"] == 0
    fam = lambda f, m=True: ok & (p["family"] == f) & m
    # one-copy records first: up to 4 columns always, 8 columns with bands 80 | 81 and PREALPS_BJ_G4_WIDE 1 | 0, never 16
    rec = q["have_g4"] == 1
    assert np.all(p["family"][ok & rec & (q["ts"] <= 4)] == G4) and not np.any(fam(G4, ~rec))
    assert np.any(fam(G4, (q["ts"] == 8) & (q["wmax"] == 80))) and not np.any(fam(G4, (q["ts"] == 8) & (q["wmax"] == 81)))
    assert not np.any(fam(G4, (q["ts"] == 8) & (q["g4_wide"] == 0))) and not np.any(fam(G4, q["ts"] == 16))
    assert np.any(fam(G4, q["R"] < 0)) and np.any(fam(G4, q["ts"] == 3))          # (asked first, whatever the class)
    rest = ok & (p["family"] != G4)
    # strides
    for ts in TS:
        assert np.any(rest & (q["ts"] == ts)) == (ts in (2, 4, 8, 16)) and np.any(~ok & (q["ts"] == ts))
    # k_bj_mfma: PREALPS_BJ_MFMA 0 | 1 | 2 against 4 | 8 columns, bands 112 | 113, tiles at 48 | 49 and 80 | 81
    narrow = (q["R"] >= 1) & (q["R"] <= 8) & (q["have_g4"] == 0)
    assert not np.any(fam(MFMA, q["mfma"] == 0)) and not np.any(fam(MFMA, (q["mfma"] == 1) & (q["ts"] <= 4)))
    assert np.all(p["family"][ok & narrow & (q["mfma"] == 2) & (q["wmax"] <= 112)] == MFMA)
    assert np.all(p["family"][ok & narrow & (q["mfma"] == 1) & (q["wmax"] <= 112) & (q["ts"] >= 8)] == MFMA)
    assert not np.any(fam(MFMA, q["wmax"] == 113)) and np.any(ok & narrow & (q["mfma"] == 2) & (q["wmax"] == 113))
    for wmax, tiles in ((0, 4), (48, 4), (49, 6), (80, 6), (81, 8), (112, 8)):
        m = fam(MFMA, q["wmax"] == wmax)
        assert m.any() and np.all(p["tiles"][m] == tiles)
    # the few-blocks split of a 4-column panel: 1023 | 1024 blocks, unknown compute units taken as 256
    four = fam(APPLY, q["ts"] == 4) | fam(PAIRS, q["ts"] == 4)
    for cus in CUS:
        assert np.all(p["ts"][four & (q["cus"] == cus) & (q["count"] <= 1023)] == 2)
        assert np.all(p["ts"][four & (q["cus"] == cus) & (q["count"] >= 1024)] == 4)
    assert np.all((p["ts"] == q["ts"])[rest & (q["ts"] != 4)])
    # paired records: classes 1 | 2, 3 | 4, with | without the records, 4 | 8 columns
    for R in range(1, 9):
        m = ok & narrow & (q["R"] == R) & (q["mfma"] == 0) & (q["have_pairs"] == 1) & (q["ts"] <= 4)
        assert m.any() and np.all(p["family"][m] == (PAIRS if R in (2, 3) else APPLY))
    assert not np.any(fam(PAIRS, q["have_pairs"] == 0)) and not np.any(fam(PAIRS, q["ts"] >= 8))
    assert np.any(fam(APPLY, np.isin(q["R"], [2, 3]) & (q["ts"] == 8))) and np.any(fam(APPLY, np.isin(q["R"], [2, 3]) & (q["have_pairs"] == 0)))
    # wavefronts per workgroup by the LDS: four, then fewer, then none
    for wmax, waves in ((319, 4), (320, 3), (415, 3), (416, 2), (639, 2), (640, 1), (1279, 1)):
        m = fam(APPLY, (q["wmax"] == wmax) & (q["have_pairs"] == 0))
        assert m.any() and np.all(p["waves"][m] == waves)
    assert np.any(fam(PAIRS, q["wmax"] == 1276)) and not np.any(fam(PAIRS, q["wmax"] == 1277))
    assert np.any(fam(APPLY, q["wmax"] == 1279)) and not np.any(fam(APPLY, q["wmax"] == 1280))
    # wide classes: 12 | 13 wavefronts, 16 | 17, per count of register sets; 16 accumulators
    for R, edges in ((1, (704, 705, 960, 961)), (2, (1472, 1473, 1984, 1985)), (4, (3008, 3009, 4032, 4033))):
        a, b, c, d = (fam(WIDE, (q["R"] == -R) & (q["wmax"] == w) & (q["ts"] == 2)) for w in edges)
        assert np.all(p["cap"][a] == 768) and np.all(p["waves"][a] == 12) and np.all(p["cap"][b] == 1024) and np.all(p["waves"][b] == 13)
        assert a.any() and b.any() and c.any() and np.all(p["waves"][c] == 16) and not d.any()
        assert np.any(fam(WIDE, (q["R"] == -R) & (q["ts"] * R == 16))) and not np.any(fam(WIDE, (q["R"] == -R) & (q["ts"] * R == 32)))
    assert not np.any(fam(WIDE, q["R"] == -3)) and not np.any(fam(WIDE, q["R"] >= 0))
    # classes 0 | 1, 8 | 9
    assert not np.any(rest & np.isin(q["R"], [0, 9])) and np.any(rest & (q["R"] == 1)) and np.any(rest & (q["R"] == 8))


def test_no_class_of_the_layout_is_refused_for_lack_of_lds(exe, tmp_path):
    """What pa_bj_layout_build (bj_build.c) can put in a class: narrow bands w <= wide_from <= 64 * 8 - 64 in class
    R = (w + 127) / 64 -- so a class R has 64 R - 127 <= wmax <= 64 R - 64 -- and wide bands in -1 / -2 / -4 by their
    window.  None of them meets "no room in the LDS" at any stride, count or switch: only the kernel's own limits
    (the window, the accumulators) refuse."""
    narrow = [(R, w) for w in range(0, 64 * MAX_R - 64 + 1) for R in [(w + 127) // 64]]
    assert {R for R, _ in narrow} == set(range(1, MAX_R + 1))
    wide = [(-(1 if W <= 1024 else 2 if W <= 2048 else 4), w) for w in range(97, 4033, 5) for W in [int(window(w))]]
    cls = np.asarray(narrow + wide, np.int32)
    rest = _product([2, 4, 8, 16], [1, 5670], [0, 1], [0, 1], [0, 1, 2])          # ts, count, have_g4 = 0, pairs, switches
    i, j = np.meshgrid(np.arange(len(cls)), np.arange(len(rest)), indexing="ij")
    c, r = cls[i.ravel()], rest[j.ravel()]
    zero = np.zeros(len(c), np.int32)
    q = np.stack([r[:, 0], c[:, 0], c[:, 1], r[:, 1], zero, r[:, 2], r[:, 3], r[:, 4], zero + 256], axis=1)
    q, p, why = run_plans(exe, tmp_path, q)
    assert not any("LDS" in t for t in why)
    assert np.all(p["rc"][q["R"] > 0] == 0)
    no = p["rc"] == 1
    assert np.all((q["ts"] * -q["R"] > 16)[no]) and np.any(no)


def test_the_labels_of_the_gpu_test_are_what_the_planner_picks(exe, tmp_path):
    """_family() of tests/test_gpu_band_blocks.py labels that test's figures by kernel family: for the classes of every
    problem there (_classes) and t in {1, 2, 4, 8, 16}, under the default switches and the ones it models, it names the
    family the planner picks."""
    import test_gpu_band_blocks as T
    cases, rows = [], []
    for name in sorted(T.PROBLEMS):
        blocks = [(b, min(w, b - 1)) for b, w in T._main_class_last(T.PROBLEMS[name]())]
        for env in ({}, {"PREALPS_BJ_G4": "0"}, {"PREALPS_BJ_G4_WIDE": "0"}, dict(T.WAVEFRONT), dict(T.WAVEFRONT, PREALPS_BJ_G4="0")):
            classes = T._classes(blocks, dict(T.BASE_ENV, **env))
            # (paired records exist when a class R = 2, 3 is left without one-copy records: bj_build.c, class_pairs)
            have_pairs = any(cl[0] in (2, 3) and not T._g4_class(cl, env) for cl in classes)
            for cl in classes:
                for t in (1, 2, 4, 8, 16):
                    cases.append((name, env, cl[:3], t, T._family(cl, t, env, 64)))
                    rows.append([T._stride(t), cl[0], cl[1], len(cl[3]), int(T._g4_class(cl, env)), int(have_pairs),
                                 int(env.get("PREALPS_BJ_G4_WIDE", "1")), 1, 256])
    _, p, _ = run_plans(exe, tmp_path, np.asarray(rows, np.int32))
    assert np.all(p["rc"] == 0)
    seen = set()
    for i, (name, env, cl, t, label) in enumerate(cases):
        fam = int(p["family"][i])
        mine = {G4: "k_bj_g4 ", MFMA: "k_bj_mfma %d tiles" % p["tiles"][i], PAIRS: "k_bj_apply_pairs", APPLY: "k_bj_apply R=%d" % p["r"][i],
                WIDE: "k_bj_wide"}[fam]
        assert label.startswith(mine) if fam == G4 else label == mine, (name, env, cl, t, label, mine)
        assert fam != G4 or ("two column sets" in label) == (T._stride(t) == 8)
        seen.add(fam)
    assert seen == {G4, MFMA, PAIRS, APPLY, WIDE}
