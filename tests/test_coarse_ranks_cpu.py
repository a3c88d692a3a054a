"""The coarse space of several processes on the host (prealps_amd/csrc/coarse_space.c): stage (a), a rank's share from its
own rows (pa_coarse_share), the sum of the shares in rank order, and stage (b), E -> Einv (pa_coarse_invert), against
pa_coarse_build on the whole matrix.  A stand-alone program (tests/c/coarse_ranks_check.c) links the unit alone, is
compiled with AddressSanitizer + UBSan and run as a program; it cuts the rows after whole parts into 1, 2 and 3 "ranks".

With one aggregate per part every entry of E comes from one rank and the others add +0.0: E and Einv have the bits of
pa_coarse_build.  With an aggregate that spans a rank boundary the entries of its rows are sums of two shares, added
in another order than pa_coarse_build adds them: entry by entry they agree within (r + 2) eps sum |zv_i[a] a_ij Vp_j[b]|,
r the number of terms -- r - 1 additions in either order and the two roundings of a product, first order -- and the
program computes that sum itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/coarse_ranks_check.c")
    tmp = tmp_path_factory.mktemp("coarse_ranks")
    out, unit = str(tmp / "coarse_ranks_check"), str(tmp / "coarse_space.o")
    flags = ["-O1", "-g", "-std=gnu11", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "coarse_space.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "coarse_ranks_check.c"), unit, "-o", out, "-lm"])
    return out, tmp


def permuted(A, part, nparts):
    perm = np.argsort(part, kind="stable")
    B = sp.csr_matrix(A)[perm][:, perm].tocsr()
    B.sort_indices()
    rowpos = np.zeros(nparts + 1, dtype=np.int32)
    rowpos[1:] = np.cumsum(np.bincount(part, minlength=nparts))
    return B, rowpos, perm


def run_case(exe, name, A, rowpos, Vp, ranks, aggr=None, max_dofs=0, threads=0):
    prog, tmp = exe
    A = sp.csr_matrix(A)
    N, nparts, k = A.shape[0], len(rowpos) - 1, Vp.shape[1]
    naggr = 0 if aggr is None else int(np.max(aggr)) + 1
    cut = np.array([r * nparts // ranks for r in range(ranks + 1)], dtype=np.int32)
    fin, fout = str(tmp / (name + ".in")), str(tmp / (name + ".out"))
    with open(fin, "wb") as f:
        np.array([N, nparts, k, naggr, max_dofs, threads, A.nnz, ranks], dtype=np.int32).tofile(f)
        A.indptr.astype(np.int32).tofile(f)
        A.indices.astype(np.int32).tofile(f)
        A.data.astype(np.float64).tofile(f)
        np.asarray(rowpos, dtype=np.int32).tofile(f)
        if aggr is not None:
            np.asarray(aggr, dtype=np.int32).tofile(f)
        np.ascontiguousarray(Vp, dtype=np.float64).tofile(f)
        cut.tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([prog, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    raw = open(fout, "rb").read()
    o = {"rc": int(np.frombuffer(raw, np.int32, 1)[0]), "msg": raw[4:260].split(b"\0")[0].decode(), "cut": cut}
    o["nc"], o["naggr"] = (int(v) for v in np.frombuffer(raw, np.int32, 2, 260))
    off = 268
    o["part_aggregate"] = np.frombuffer(raw, np.int32, nparts, off); off += 4 * nparts
    o["per_rank"] = np.frombuffer(raw, np.int32, ranks, off); off += 4 * ranks
    o["ranks"] = []
    if o["rc"] == 0:
        nc = o["nc"]
        for _ in range(ranks):
            m, nch, nrows = (int(v) for v in np.frombuffer(raw, np.int32, 3, off)); off += 12
            r = {"m": m}
            for key, n in (("ch_row0", nch), ("ch_nrows", nch), ("ch_aggr", nch), ("agg_ptr", o["naggr"] + 1), ("agg_chunk", nch),
                           ("rows", nrows)):
                r[key] = np.frombuffer(raw, np.int32, n, off); off += 4 * n
            r["zv"] = np.frombuffer(raw, np.float64, m * k, off).reshape(m, k); off += 8 * m * k
            o["ranks"].append(r)
        for key in ("E", "Einv", "E_whole", "Einv_whole", "Eabs", "terms"):
            o[key] = np.frombuffer(raw, np.float64, nc * nc, off).reshape(nc, nc); off += 8 * nc * nc
        assert off == len(raw)
    return o


def check_shares(o, rowpos, aggr, Vp, CH=1024):
    """What every rank holds: zv of its rows, the chunks of its parts counted from its first row, a chunk list for every
    aggregate -- empty where it has no chunk -- and the coarse rows of exactly the aggregates that have one."""
    k, aggr = Vp.shape[1], np.asarray(aggr)
    for r, sh in enumerate(o["ranks"]):
        p0, p1 = int(o["cut"][r]), int(o["cut"][r + 1])
        r0 = int(rowpos[p0])
        assert sh["m"] == rowpos[p1] - r0 and np.array_equal(sh["zv"], Vp[r0:rowpos[p1]])
        want = [(x - r0, min(CH, rowpos[p + 1] - x), aggr[p]) for p in range(p0, p1) for x in range(rowpos[p], rowpos[p + 1], CH)]
        assert list(zip(sh["ch_row0"], sh["ch_nrows"], sh["ch_aggr"])) == [tuple(int(v) for v in w) for w in want]
        here = set(int(g) for g in aggr[p0:p1])
        for g in range(o["naggr"]):
            lst = sh["agg_chunk"][sh["agg_ptr"][g]:sh["agg_ptr"][g + 1]]
            assert np.array_equal(lst, np.flatnonzero(sh["ch_aggr"] == g))             # ascending, complete
            assert (len(lst) > 0) == (g in here)                                          # absent: an empty list
        assert np.array_equal(sh["rows"], [g * k + a for g in sorted(here) for a in range(k)])


def _poisson():
    from prealps_amd.gen import box_partition, poisson3d_csr
    rp, ci, v = poisson3d_csr(8)
    A = sp.csr_matrix((v, ci, rp), shape=(512, 512))
    part, nparts = box_partition(8, (4, 4, 2))
    assert nparts == 16
    B, rowpos, perm = permuted(A, part, nparts)
    V = np.random.default_rng(81).standard_normal((512, 3))
    V[:, 0] = 1.0
    return B, rowpos, V[perm]


def _elasticity():
    from prealps_amd.gen import box_partition_nodes, elasticity3d_csr
    from prealps_amd.nearkernel import translations
    nn = (6, 5, 5)
    rp, ci, v = elasticity3d_csr(nn)
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    part, nparts = box_partition_nodes(nn, (2, 2, 2))
    B, rowpos, perm = permuted(A, part, nparts)
    return B, rowpos, translations(N, 3)[perm]


_PROBLEMS = {"poisson": _poisson, "elasticity": _elasticity}
_made = {}


def _problem(name):
    if name not in _made:
        _made[name] = _PROBLEMS[name]()
    return _made[name]


@pytest.mark.parametrize("ranks", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["poisson", "elasticity"])
def test_one_aggregate_per_part_has_the_bits_of_the_whole_build(exe, name, k, ranks):
    B, rowpos, V = _problem(name)
    Vp = np.ascontiguousarray(V[:, :k])
    nparts = len(rowpos) - 1
    aggr = np.arange(nparts)
    o = run_case(exe, "%s_one_k%d_r%d" % (name, k, ranks), B, rowpos, Vp, ranks, aggr=aggr)
    assert o["rc"] == 0, o["msg"]
    assert o["nc"] == nparts * k
    check_shares(o, rowpos, aggr, Vp)
    assert o["E"].tobytes() == o["E_whole"].tobytes()
    assert o["Einv"].tobytes() == o["Einv_whole"].tobytes()
    assert np.array_equal(o["Einv"], o["Einv"].T)


def _spanning(nparts, cut):
    """Aggregates of two or three consecutive parts, numbered without gaps, one of which spans a rank boundary."""
    for s in range(3):
        aggr = (np.arange(nparts) + s) // 3
        if any(aggr[c - 1] == aggr[c] for c in cut[1:-1]):
            return aggr
    raise AssertionError("no shift makes an aggregate span a boundary")


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["poisson", "elasticity"])
def test_an_aggregate_that_spans_ranks_within_the_rounding_of_its_terms(exe, name, k, ranks):
    B, rowpos, V = _problem(name)
    Vp = np.ascontiguousarray(V[:, :k])
    nparts = len(rowpos) - 1
    cut = [r * nparts // ranks for r in range(ranks + 1)]
    aggr = _spanning(nparts, cut)
    assert len(np.unique(aggr)) == aggr.max() + 1 and np.bincount(aggr).max() <= 3
    o = run_case(exe, "%s_span_k%d_r%d" % (name, k, ranks), B, rowpos, Vp, ranks, aggr=aggr)
    assert o["rc"] == 0, o["msg"]
    check_shares(o, rowpos, aggr, Vp)
    # the rows of a spanning aggregate are listed on both sides of the boundary
    shared = [g for g in range(o["naggr"]) if sum(g * k in sh["rows"] for sh in o["ranks"]) > 1]
    assert shared
    bound = (o["terms"] + 2) * EPS * o["Eabs"]
    err = np.abs(o["E"] - o["E_whole"])
    asym = np.abs(o["E"] - o["E"].T)
    nz = bound > 0
    print("%s k %d ranks %d: %d shared aggregates, largest |E - E_whole| / bound %.3e, largest |E - E^T| / bound %.3e, most terms %d"
          % (name, k, ranks, len(shared), (err[nz] / bound[nz]).max(), (asym[nz] / bound[nz]).max(), int(o["terms"].max())))
    assert (err <= bound).all()
    assert (asym <= bound).all()
    # Einv: the inverse of that E
    cond = np.linalg.cond(o["E_whole"])
    assert np.abs(o["Einv"] @ o["E_whole"] - np.eye(o["nc"])).max() <= 100 * o["nc"] * EPS * cond
    assert np.array_equal(o["Einv"], o["Einv"].T)


def test_default_aggregates_over_the_cap_are_cut_rank_by_rank(exe):
    """48 one-row parts, one vector, a cap of 10 unknowns, 3 ranks: floor(10 * 16 / 48) = 3 aggregates per rank."""
    n = 48
    A = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    rowpos = np.arange(n + 1, dtype=np.int32)
    Vp = np.ones((n, 1))
    o = run_case(exe, "default48", A, rowpos, Vp, 3, max_dofs=10)
    assert o["rc"] == 0, o["msg"]
    assert list(o["per_rank"]) == [3, 3, 3] and o["naggr"] == 9 and o["nc"] == 9
    agg = o["part_aggregate"]
    assert np.array_equal(np.unique(agg), np.arange(9))                                 # numbered without gaps
    for r in range(3):                                                                    # no aggregate spans ranks
        mine = agg[16 * r:16 * (r + 1)]
        assert mine.min() == 3 * r and mine.max() == 3 * r + 2
    check_shares(o, rowpos, agg, Vp)
    for r, sh in enumerate(o["ranks"]):
        assert np.array_equal(sh["rows"], [3 * r, 3 * r + 1, 3 * r + 2])
    # every entry of E comes from one rank: the bits of the whole build
    assert o["E"].tobytes() == o["E_whole"].tobytes() and o["Einv"].tobytes() == o["Einv_whole"].tobytes()
    # under the cap: one aggregate per part whatever the ranks
    o = run_case(exe, "default48_fits", A, rowpos, Vp, 3, max_dofs=48)
    assert o["rc"] == 0 and list(o["per_rank"]) == [16, 16, 16] and np.array_equal(o["part_aggregate"], np.arange(48))


def test_a_singular_sum_names_aggregate_and_vector(exe):
    B, rowpos, V = _problem("poisson")
    Vp = np.ascontiguousarray(V[:, :2]).copy()
    Vp[:, 1] = Vp[:, 0]
    nparts = len(rowpos) - 1
    o = run_case(exe, "dependent_r2", B, rowpos, Vp, 2, aggr=np.arange(nparts))
    assert o["rc"] == 1004 and "aggregate 0, vector 1" in o["msg"]
