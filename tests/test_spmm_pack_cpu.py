"""The packed form of the run plan's value array (prealps_amd/csrc/spmm_pack.c) is host arithmetic: a stand-alone
program (tests/c/spmm_pack_dump.c) cuts the run plan of small matrices under AddressSanitizer + UBSan, packs its
values, and checks that masks + kept values reproduce the plan's value array bit for bit, that pack_pos is strictly
increasing and consistent with the masks, and that lanes beyond a slice's rows hold nothing.  The counts it prints
are held against the matrices here."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
NEGZEROS = 5


def _write(path, A, rowpos):
    A = sp.csr_matrix(A)
    with open(path, "wb") as f:
        np.array([A.shape[0], len(rowpos) - 1, A.nnz], dtype=np.int32).tofile(f)
        np.asarray(rowpos, dtype=np.int32).tofile(f)
        A.indptr.astype(np.int32).tofile(f)
        A.indices.astype(np.int32).tofile(f)
        A.data.astype(np.float64).tofile(f)


def _csr_keeping_zeros(rp, ci, v):
    n = len(rp) - 1
    return sp.csr_matrix((v.copy(), ci.copy(), rp.copy()), shape=(n, n))


def _cases():
    """name -> (matrix with its stored zeros, first row of every part)."""
    from prealps_amd import gen
    out = {}
    rp, ci, v = gen.elasticity3d_csr(7)
    n = len(rp) - 1
    cut8 = [(p * n) // 8 for p in range(9)]                  # 8 contiguous parts: nodes are cut apart
    out["elasticity7_cut8"] = (_csr_keeping_zeros(rp, ci, v), cut8)
    nn = (12, 10, 10)
    rp2, ci2, v2 = gen.elasticity3d_csr(nn)
    part, P = gen.box_partition_nodes(nn, (2, 2, 2))
    perm = np.argsort(part, kind="stable")
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    rows = np.repeat(np.arange(len(rp2) - 1), np.diff(rp2))
    order = np.lexsort((inv[ci2], inv[rows]))                # P A P^T entry by entry: the stored zeros stay
    B = sp.csr_matrix((v2[order], inv[ci2][order], np.concatenate(([0], np.cumsum(np.bincount(inv[rows], minlength=len(perm)))))),
                      shape=(len(perm), len(perm)))
    out["elasticity12_boxes"] = (B, np.concatenate(([0], np.cumsum(np.bincount(part, minlength=P)))))
    full = v.copy()
    full[full.view(np.uint64) == 0] = 0.25                   # no stored zero at all
    out["no_zero"] = (_csr_keeping_zeros(rp, ci, full), cut8)
    third = full.copy()
    third[ci % 3 == 2] = 0.0                                 # the third dof of every node: a whole position is empty
    out["empty_position"] = (_csr_keeping_zeros(rp, ci, third), [0, n // 2, n])
    neg = v.copy()
    zeros = np.flatnonzero(neg.view(np.uint64) == 0)
    neg[zeros[:: len(zeros) // NEGZEROS][:NEGZEROS]] = -0.0   # stored -0.0: a value like any other
    out["negative_zero"] = (_csr_keeping_zeros(rp, ci, neg), cut8)
    return out


def _build(tmp, defines):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/spmm_pack_dump.c")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    exe, plan, pack = str(tmp / "spmm_pack_dump"), str(tmp / "spmm_plan.o"), str(tmp / "spmm_pack.o")
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "spmm_plan.c"), "-o", plan])
    subprocess.check_call([gcc] + flags + defines + ["-c", os.path.join(CSRC, "spmm_pack.c"), "-o", pack])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "spmm_pack_dump.c"), plan, pack, "-o", exe])
    return exe


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or pack failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout.splitlines()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("spmm_pack_cases")
    files = {}
    for name, (A, rowpos) in _cases().items():
        files[name] = (str(tmp / name), A)
        _write(files[name][0], A, rowpos)
    return files


@pytest.fixture(scope="module")
def report(cases, tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("spmm_pack"), [])
    lines = _run(exe, [path for path, _ in cases.values()])
    out = {}
    for line in lines:
        name, rest = line.split(": ", 1)
        assert rest.startswith("ok "), line
        out[name] = {k: float(x) for k, x in (kv.split("=") for kv in rest.split()[1:])}
    assert set(out) == set(cases)
    return out


def test_unpacked_values_are_the_plans_and_the_counts_are_the_matrixs(cases, report):
    """(the program has compared the unpacked array with the plan's, bit for bit)  Every entry of the panel is
    stored once in a run plan, so the kept values are the entries whose bits are not those of +0.0."""
    for name, (_, A) in cases.items():
        r = report[name]
        assert r["runs"] == 1 and r["stored"] == 192 * r["steps"]
        assert r["kept"] == np.count_nonzero(A.data.view(np.uint64)), name
        assert r["packed_bytes"] == 8 * (r["kept"] + r["steps"]) + 32 * r["steps"]
        assert r["unpacked_bytes"] == 8 * r["stored"]
        print("%s: %d of %d stored values kept, %.3f of the bytes" % (name, r["kept"], r["stored"],
                                                                      r["packed_bytes"] / r["unpacked_bytes"]))


def test_the_cases_reach_what_they_are_there_for(cases, report):
    assert report["elasticity7_cut8"]["min_slice_rows"] < 64                   # nodes cut apart, short last slices
    assert report["elasticity12_boxes"]["min_slice_rows"] == 24                # slices of 24 rows ...
    # ... four of them in a block, the most pa_spmm_plan_build cuts (a block has at most 256 / 64 slices, however
    # short they are), so the wavefronts of a workgroup all have a slice; the pack itself knows no blocks
    assert report["elasticity12_boxes"]["max_block_slices"] == 4
    A = cases["no_zero"][1]
    assert np.count_nonzero(A.data.view(np.uint64)) == A.nnz
    assert report["no_zero"]["kept"] == A.nnz
    assert report["empty_position"]["empty_masks"] > report["no_zero"]["empty_masks"] + report["empty_position"]["steps"] / 2
    assert report["negative_zero"]["negzeros"] == NEGZEROS and report["elasticity7_cut8"]["negzeros"] == 0
    assert report["negative_zero"]["kept"] == report["elasticity7_cut8"]["kept"] + NEGZEROS
    # Q1 elasticity stores whole element matrices: more than a third of the stored values are +0.0
    assert report["elasticity12_boxes"]["kept"] < 0.67 * report["elasticity12_boxes"]["stored"]


def test_every_failed_allocation_is_reported_and_released(cases, tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("spmm_pack_fail"), ["-Dmalloc=t_malloc"])
    lines = _run(exe, ["fail-allocs"] + [path for path, _ in cases.values()])
    assert len(lines) == len(cases) and all("every failed allocation handled" in l for l in lines)
