"""The 2-byte codes of the packed run plan (prealps_amd/csrc/spmm_code.c) are host arithmetic: a stand-alone program
(tests/c/spmm_code_dump.c) cuts the run plan of small matrices under AddressSanitizer + UBSan, packs and codes its
values and checks the coded form element by element (table[code] has the packed value's bits, entry 0 is +0.0, no
pattern twice, counts do not increase, raw blocks have empty tables).  What it dumps is restated here with numpy from
the plan's own arrays: the tables (distinct bit patterns per block, most frequent first, ties by bit pattern), the fit
rule, the byte counts and the statistics."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import spmm_code_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
BUDGET = 32768                                       # the LDS of a workgroup at up to 4 columns (five per CU)


def _write(path, A, rowpos):
    with open(path, "wb") as f:
        np.array([A.shape[0], len(rowpos) - 1, A.nnz], dtype=np.int32).tofile(f)
        np.asarray(rowpos, dtype=np.int32).tofile(f)
        A.indptr.astype(np.int32).tofile(f)
        A.indices.astype(np.int32).tofile(f)
        A.data.astype(np.float64).tofile(f)


def _panel(rp, ci, v, P, part):
    """P A P^T entry by entry with the parts contiguous (the stored zeros stay), and the first row of every part."""
    perm = np.argsort(part, kind="stable")
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    order = np.lexsort((inv[ci], inv[rows]))
    n = len(perm)
    B = sp.csr_matrix((v[order], inv[ci][order], np.concatenate(([0], np.cumsum(np.bincount(inv[rows], minlength=n))))), shape=(n, n))
    return B, np.concatenate(([0], np.cumsum(np.bincount(part, minlength=P))))


def _cases():
    """name -> (panel, rowpos, ts, budget)"""
    out = {}
    rp7, ci7, v7, P7, part7 = K.base("elasticity7")
    rp12, ci12, v12, P12, part12 = K.base("elasticity12")
    n12 = len(rp12) - 1
    out["elasticity7_cut8"] = _panel(rp7, ci7, v7, P7, part7) + (4, BUDGET)
    out["elasticity12_boxes"] = _panel(rp12, ci12, v12, P12, part12) + (4, BUDGET)
    out["elasticity12_ts2"] = _panel(rp12, ci12, v12, P12, part12) + (2, BUDGET)
    out["elasticity7_distinct"] = _panel(rp7, ci7, K.distinct(v7), P7, part7) + (4, BUDGET)
    out["elasticity12_distinct"] = _panel(rp12, ci12, K.distinct(v12), P12, part12) + (4, BUDGET)
    # (the same with room for every table: what a forced plan codes when it fits)
    out["elasticity12_distinct_roomy"] = _panel(rp12, ci12, K.distinct(v12), P12, part12) + (4, 1 << 20)
    # the factors go on a contiguous quarter of the rows of the panel: the blocks there lose their repetition
    B, rowpos = _panel(rp12, ci12, v12, P12, part12)
    B = sp.csr_matrix((K.mixed(B.indptr, B.data, n12 // 4, n12 // 2), B.indices, B.indptr), shape=B.shape)
    out["elasticity12_mixed"] = (B, rowpos, 4, BUDGET)
    out["elasticity7_special"] = _panel(rp7, ci7, K.special(rp7, ci7, v7), P7, part7) + (4, BUDGET)
    return out


def _build(tmp, defines):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/spmm_code_dump.c")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    exe = str(tmp / "spmm_code_dump")
    objs = []
    for unit, extra in (("spmm_plan", []), ("spmm_pack", []), ("spmm_code", defines)):
        objs.append(str(tmp / (unit + ".o")))
        subprocess.check_call([gcc] + flags + extra + ["-c", os.path.join(CSRC, unit + ".c"), "-o", objs[-1]])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "spmm_code_dump.c")] + objs + ["-o", exe])
    return exe


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or code failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout.splitlines()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("spmm_code_cases")
    files = {}
    for name, (A, rowpos, ts, budget) in _cases().items():
        files[name] = (str(tmp / name), A, ts, budget)
        _write(files[name][0], A, rowpos)
    return files


def _load(path):
    with open(path, "rb") as f:
        nblk, ncode, ntab = np.fromfile(f, dtype=np.int64, count=3)
        blk = np.fromfile(f, dtype=np.int64, count=4 * nblk).reshape(nblk, 4)
        off = np.fromfile(f, dtype=np.int64, count=nblk + 1)
        val = np.fromfile(f, dtype=np.uint64, count=ncode)
        code = np.fromfile(f, dtype=np.uint16, count=ncode)
        tab = np.fromfile(f, dtype=np.uint64, count=ntab)
    return {"blk": blk, "off": off, "val": val, "code": code, "tab": tab}


@pytest.fixture(scope="module")
def report(cases, tmp_path_factory):
    """name -> (the counts the program printed, what it dumped); the program has checked every element itself."""
    tmp = tmp_path_factory.mktemp("spmm_code")
    exe = _build(tmp, [])
    out = {}
    for name, (path, _, ts, budget) in cases.items():
        dump = str(tmp / (name + ".bin"))
        lines = _run(exe, [str(ts), str(budget), path, dump])
        assert len(lines) == 1 and lines[0].startswith(name + ": ok "), lines
        out[name] = ({k: float(x) for k, x in (kv.split("=") for kv in lines[0].split()[2:])}, _load(dump))
    return out


def _expected_table(bits):
    """+0.0, then the other distinct patterns of the block: most frequent first, ties by ascending bit pattern"""
    u, c = np.unique(bits[bits != 0], return_counts=True)
    order = np.lexsort((u, -c))
    return np.concatenate((np.zeros(1, dtype=np.uint64), u[order]))


def test_tables_fit_rule_and_bytes_against_numpy(cases, report):
    for name, (_, _, ts, budget) in cases.items():
        r, d = report[name]
        coded_elems = entries = ncoded = lds = 0
        for b, (e0, e1, nown, nxt) in enumerate(d["blk"]):
            bits = d["val"][e0:e1]
            want = _expected_table(bits)
            need = (nown + nxt + 2) * ts * 8 + 8 * len(want)
            fits = need <= budget and len(want) <= 65536
            got = d["tab"][d["off"][b]:d["off"][b + 1]]
            if not fits:
                assert len(got) == 0 and not d["code"][e0:e1].any(), (name, b)       # raw: an empty table, codes 0
                continue
            assert np.array_equal(got, want), (name, b)
            assert np.array_equal(got[d["code"][e0:e1]], bits), (name, b)           # every element decodes to its bits
            ncoded += 1
            coded_elems += e1 - e0
            entries += len(want)
            lds = max(lds, need)
        end = d["blk"][-1][1]
        assert end == r["steps"] + r["kept"] and not d["code"][end:].any() and len(d["code"]) == end + 64     # the slack
        assert (r["ncoded"], r["ntab"], r["coded_elems"], r["lds"]) == (ncoded, entries, coded_elems, lds), name
        assert r["packed_bytes"] == 8 * (r["kept"] + r["steps"]) + 32 * r["steps"]
        assert r["coded_bytes"] == r["packed_bytes"] - 6 * coded_elems + 8 * entries, name
        assert lds <= budget and r["stage_cap"] * ts * 8 <= BUDGET
        print("%s: %d of %d blocks coded, %d table entries, values %.0f -> %.0f bytes" % (
            name, ncoded, r["nblk"], entries, r["packed_bytes"], r["coded_bytes"]))


def _passes_rule(r):
    """operator.c: coded when the coded plan streams less than 0.9 of what the packed plan streams"""
    packed = r["stream_bytes"] - r["unpacked_bytes"] + r["packed_bytes"]
    return r["ncoded"] > 0 and packed - r["packed_bytes"] + r["coded_bytes"] < 0.9 * packed


def test_the_cases_reach_what_they_are_there_for(cases, report):
    for name in ("elasticity7_cut8", "elasticity12_boxes", "elasticity12_ts2"):
        r, d = report[name]
        assert r["runs"] == 1 and r["ncoded"] == r["nblk"] > 1 and _passes_rule(r), name       # everything coded ...
        assert r["ntab"] <= 64 * r["nblk"], name                                               # ... few entries per table
        assert r["coded_bytes"] < 0.5 * r["packed_bytes"], name
    # no repetition: nothing passes the rule; what a forced plan codes (the blocks that fit) decodes exactly (above)
    for name in ("elasticity7_distinct", "elasticity12_distinct", "elasticity12_distinct_roomy"):
        r, d = report[name]
        assert not _passes_rule(r), name
        kept = sum(int(np.count_nonzero(d["val"][e0:e1])) for b, (e0, e1, _, _) in enumerate(d["blk"]) if d["off"][b + 1] > d["off"][b])
        assert r["ntab"] == r["ncoded"] + kept, name                                           # a code of its own per value
    assert report["elasticity12_distinct"][0]["ncoded"] < report["elasticity12_distinct"][0]["nblk"]        # tables beyond the LDS
    r = report["elasticity12_distinct_roomy"][0]
    assert r["ncoded"] == r["nblk"] and r["ntab"] == r["kept"] + r["nblk"] and r["lds"] > BUDGET
    # coded and raw blocks in one plan, and the plan as a whole passes the rule
    r, d = report["elasticity12_mixed"]
    assert 0 < r["ncoded"] < r["nblk"] and _passes_rule(r)
    sizes = np.diff(d["off"])
    assert (sizes == 0).sum() == r["nblk"] - r["ncoded"] and sizes[sizes > 0].min() <= 64


def test_special_patterns_are_kept_apart_bit_by_bit(report):
    r, d = report["elasticity7_special"]
    assert r["ncoded"] == r["nblk"]
    pats = {"-0.0": np.uint64(0x8000000000000000), "denormal": np.array([K.DENORMAL]).view(np.uint64)[0],
            "nan_a": np.array([K.NAN_A]).view(np.uint64)[0], "nan_b": np.array([K.NAN_B]).view(np.uint64)[0]}
    assert (d["val"] == pats["-0.0"]).sum() == K.SPECIAL_NEGZEROS
    for what, p in pats.items():
        at = np.flatnonzero(d["val"] == p)
        assert len(at) >= 1, what
        for i in at:                                                       # a code that is not 0, and a table entry with these bits
            b = int(np.searchsorted(d["blk"][:, 1], i, side="right"))
            assert d["code"][i] != 0 and d["tab"][d["off"][b] + d["code"][i]] == p, what
    # the two NaNs share a block here or not: either way they are two entries
    assert pats["nan_a"] != pats["nan_b"] and (d["tab"] == pats["nan_a"]).sum() == (d["tab"] == pats["nan_b"]).sum() == 1


def test_every_failed_allocation_is_reported_and_released(cases, tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("spmm_code_fail"), ["-Dmalloc=t_malloc"])
    for name in ("elasticity12_boxes", "elasticity12_mixed", "elasticity12_distinct_roomy"):       # (the last one grows its tables)
        path, _, ts, budget = cases[name]
        lines = _run(exe, ["fail-allocs", str(ts), str(budget), path])
        assert len(lines) == 1 and "every failed allocation handled" in lines[0], lines
    assert int(lines[0].rsplit("(", 1)[1].rstrip(")")) > 4                  # the growing table's allocations failed too
