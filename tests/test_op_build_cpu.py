"""The shard of one process (prealps_amd/csrc/op_build.c: ordering, scaling vector, row panel, halo slots, send lists)
is plain host arithmetic: a stand-alone program (tests/c/op_build_check.c) links the unit alone, is compiled with
AddressSanitizer + UBSan and run as a program.  It prints the shard of every rank; every array is restated here with
numpy, independently of the C code, and compared exactly (integers and the bits of the doubles)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from prealps_amd import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
OK, NOMEM, DIAG, SCALE, PART, DUP = 0, -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/op_build_check.c")
    tmp = tmp_path_factory.mktemp("op_build")
    out, unit = str(tmp / "op_build_check"), str(tmp / "op_build.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "op_build.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "op_build_check.c"), unit, "-lm", "-o", out])
    return out


def test_the_unit_includes_its_own_header_the_allocation_header_and_libc_only():
    src = open(os.path.join(CSRC, "op_build.c")).read() + open(os.path.join(CSRC, "op_build.h")).read()
    includes = set(line.split()[1] for line in src.splitlines() if line.startswith("#include"))
    assert includes == {'"op_build.h"', '"pa_alloc.h"', "<math.h>", "<omp.h>", "<stddef.h>", "<stdio.h>", "<stdlib.h>",
                        "<string.h>"}
    assert "getenv" not in src and "pa_host.h" not in src
    alloc = open(os.path.join(CSRC, "pa_alloc.h")).read()
    assert set(line.split()[1] for line in alloc.splitlines() if line.startswith("#include")) == \
        {"<stddef.h>", "<stdlib.h>", "<sys/mman.h>"}


def matrix(kind):
    """Poisson 6^3, or the one-sided pattern of test_mpi_cpu.py on it (`general`, not structurally symmetric)."""
    n = 6
    rp, ci, v = gen.poisson3d_csr(n)
    if kind == "unsym":
        A0 = sp.coo_matrix(sp.csr_matrix((v, ci, rp), shape=(n ** 3, n ** 3)))
        keep = ~((A0.row > A0.col) & ((A0.row + A0.col) % 3 == 0))
        A0 = sp.csr_matrix((A0.data[keep] * (1.0 + 0.01 * (A0.row[keep] % 7)), (A0.row[keep], A0.col[keep])), shape=A0.shape)
        A0.sort_indices()
        rp, ci, v = A0.indptr, A0.indices, A0.data
    return np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(v, np.float64)


def random_part(N, nparts, seed):
    rng = np.random.default_rng(seed)
    part = rng.integers(0, nparts, N)
    part[rng.permutation(N)[:nparts]] = np.arange(nparts)      # no empty part
    return part


def run(exe, path, rp, ci, v, size, nparts, part, scale, keep_src, threads):
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d %d\n" % (len(rp) - 1, len(ci), size, nparts, part is not None, scale, keep_src, threads))
        f.write(" ".join(str(int(x)) for x in rp) + "\n" + " ".join(str(int(x)) for x in ci) + "\n")
        f.write(" ".join(repr(float(x)) for x in v) + "\n")
        if part is not None:
            f.write(" ".join(str(int(x)) for x in part) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", "sanitizer or program failure:\n" + r.stderr[-4000:]
    return r.stdout


def parse(out):
    """One dict per rank: arrays by name, or {"error": (code, message), "empty": flag}."""
    ranks = []
    for line in out.splitlines():
        name, _, rest = line.partition(" ")
        if name == "rank":
            ranks.append({})
        elif name == "error":
            code, _, msg = rest.partition(" ")
            ranks[-1]["error"] = (int(code), msg)
        elif name in ("empty", "whole0", "values"):
            ranks[-1][name] = int(rest)
        else:
            f = rest.split()
            assert len(f) == int(f[0]) + 1, name
            ranks[-1][name] = np.array(f[1:], dtype=np.float64 if name in ("d", "val") else np.int64)
    return ranks


def expected(rp, ci, v, size, nparts, part, scale, keep_src, rank):
    """The shard of `rank` from its definition: the panel as rows of P (D A D) P^T, and what follows from it."""
    N = len(rp) - 1
    rows = np.repeat(np.arange(N), np.diff(rp))
    p = part if part is not None else np.arange(N) * nparts // N
    perm = np.argsort(p, kind="stable")                      # rows grouped part by part, original order inside
    iperm = np.empty(N, np.int64); iperm[perm] = np.arange(N)
    rowPos = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=nparts))])
    d = None
    if scale:
        mx = np.zeros(N); np.maximum.at(mx, rows, np.abs(v))
        d = np.sqrt(1.0 / mx)
    first = [g * nparts // size for g in range(size + 1)]     # process g owns parts [first[g], first[g + 1])
    lo, hi = rowPos[first[rank]], rowPos[first[rank + 1]]
    m = hi - lo
    vals = (d[rows] * v) * d[ci] if scale else v
    nr, nc = iperm[rows], iperm[ci]
    order = np.lexsort((nc, nr))
    order = order[(nr[order] >= lo) & (nr[order] < hi)]
    colInd, val, src = nc[order], vals[order], order
    rowPtr = np.concatenate([[0], np.cumsum(np.bincount(nr[order] - lo, minlength=m))])
    off = (colInd < lo) | (colInd >= hi)
    halo_cols = np.unique(colInd[off])
    lcol = np.where(off, m + np.searchsorted(halo_cols, colInd), colInd - lo)
    owner_of_row = np.searchsorted(rowPos[first], np.arange(N), side="right") - 1      # new row -> process
    recv_by_proc = np.bincount(owner_of_row[halo_cols], minlength=size)
    send = []                                                 # per process g: the rows of ours that g's rows name as columns
    for g in range(size):
        theirs = (owner_of_row[nr] == g) & (nc >= lo) & (nc < hi)
        send.append(np.unique(nc[theirs]) - lo if g != rank else np.zeros(0, np.int64))
    peers = [g for g in range(size) if len(send[g]) or recv_by_proc[g]]
    send_idx = np.concatenate(send) if size else np.zeros(0, np.int64)
    slots = [np.flatnonzero(send_idx == r) for r in range(m)]
    e = {"head": np.array([N, nparts, first[rank], first[rank + 1], lo, m, len(colInd), len(halo_cols), len(peers), len(send_idx)]),
         "rowPos": rowPos, "perm": perm, "iperm": iperm, "d": d if scale else np.zeros(0), "rowPtr": rowPtr,
         "colInd": colInd, "val": val, "src": src if keep_src else np.zeros(0, np.int64),
         "lcol": np.concatenate([lcol, np.zeros(8, np.int64)]), "halo_cols": halo_cols, "recv_by_proc": recv_by_proc,
         "peers": np.array(peers, np.int64), "send_rows": np.array([len(send[g]) for g in peers], np.int64),
         "recv_rows": np.array([recv_by_proc[g] for g in peers], np.int64), "send_idx": send_idx,
         "pk_off": np.concatenate([[0], np.cumsum([len(s) for s in slots])]),
         "pk_slot": np.concatenate(slots) if m else np.zeros(0, np.int64)}
    return e


@pytest.mark.parametrize("kind", ["poisson", "unsym"])
@pytest.mark.parametrize("size,nparts", [(1, 1), (1, 7), (2, 2), (2, 7), (3, 3), (3, 7)])
@pytest.mark.parametrize("partition", ["contiguous", "random"])
def test_shards_match_their_definition(exe, tmp_path, kind, size, nparts, partition):
    rp, ci, v = matrix(kind)
    part = random_part(len(rp) - 1, nparts, 11 + nparts) if partition == "random" else None
    for scale, keep_src in itertools.product([0, 1], [0, 1]):
        out = run(exe, str(tmp_path / "case.txt"), rp, ci, v, size, nparts, part, scale, keep_src, 1)
        assert out == run(exe, str(tmp_path / "case4.txt"), rp, ci, v, size, nparts, part, scale, keep_src, 4)   # threads
        got = parse(out)
        assert len(got) == size
        rows = 0
        for rank in range(size):
            g, e = got[rank], expected(rp, ci, v, size, nparts, part, scale, keep_src, rank)
            assert "error" not in g, g
            for name, want in e.items():
                assert g[name].dtype == want.dtype or len(want) == 0, name
                np.testing.assert_array_equal(g[name], want, err_msg="%s of rank %d" % (name, rank))   # doubles: by ==
            if keep_src:      # src: d[old] * val[src[e]] * d[col] is the panel value, bit for bit
                old = e["perm"][e["head"][4] + np.repeat(np.arange(e["head"][5]), np.diff(g["rowPtr"]))]
                col = e["perm"][g["colInd"]]
                again = (g["d"][old] * v[g["src"]]) * g["d"][col] if scale else v[g["src"]]
                assert np.array_equal(again, g["val"])
            assert g["whole0"] == 1 and g["values"] == 1
            # the inverse send list inverts send_idx
            for r in range(e["head"][5]):
                s = g["pk_slot"][g["pk_off"][r]:g["pk_off"][r + 1]]
                assert np.all(g["send_idx"][s] == r) and np.all(np.diff(s) > 0)
            assert g["pk_off"][-1] == len(g["send_idx"])
            rows += e["head"][5]
        assert rows == len(rp) - 1


def test_errors_leave_an_empty_shard(exe, tmp_path):
    rp, ci, v = matrix("poisson")
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    path = str(tmp_path / "bad.txt")

    def first_error(out):
        errs = [g for g in parse(out) if "error" in g]
        assert errs and all(g["empty"] == 1 for g in errs)
        return errs

    # a missing diagonal in two rows: the message names the lower
    B = sp.lil_matrix(A); B[17, 17] = 0; B[5, 5] = 0
    B = sp.csr_matrix(B); B.eliminate_zeros()
    for threads in (1, 4):
        errs = first_error(run(exe, path, B.indptr, B.indices, B.data, 2, 4, None, 1, 1, threads))
        assert len(errs) == 2 and all(g["error"] == (DIAG, "Diagonal is not set correctly (row 5)") for g in errs)
    # a zero row, scaled (the pattern keeps its diagonal) -- and not an error without scaling
    vz = v.copy(); vz[rp[3]:rp[4]] = 0.0
    errs = first_error(run(exe, path, rp, ci, vz, 2, 4, None, 1, 0, 1))
    assert all(g["error"] == (SCALE, "Impossible to scale the matrix, rcmin=0") for g in errs) and len(errs) == 2
    assert all("error" not in g for g in parse(run(exe, path, rp, ci, vz, 2, 4, None, 0, 0, 1)))
    # a partition entry out of range, an empty part
    part = random_part(N, 5, 3); part[7] = 5
    errs = first_error(run(exe, path, rp, ci, v, 1, 5, part, 1, 1, 1))
    assert errs[0]["error"] == (PART, "partition entry 5 of row 7 out of range")
    part[7] = -1
    assert first_error(run(exe, path, rp, ci, v, 1, 5, part, 1, 1, 1))[0]["error"] == (PART, "partition entry -1 of row 7 out of range")
    part = random_part(N, 5, 3); part[part == 2] = 3
    errs = first_error(run(exe, path, rp, ci, v, 3, 5, part, 0, 0, 1))
    assert len(errs) == 3 and all(g["error"] == (PART, "part 2 is empty") for g in errs)
    # a row holding one column twice: the rank that owns the row refuses, the other builds its shard
    k = rp[4]
    ci2, v2 = np.insert(ci, k, ci[k + 1]), np.insert(v, k, 0.5)
    rp2 = rp.copy(); rp2[5:] += 1
    msg = "row 4 holds the same column twice: sum duplicate entries before building the operator"
    for size in (1, 2):
        got = parse(run(exe, path, rp2, ci2, v2, size, 2, None, 1, 1, 4))
        assert got[0]["error"] == (DUP, msg) and got[0]["empty"] == 1
        assert all("error" not in g for g in got[1:])
