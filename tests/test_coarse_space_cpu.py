"""The host unit of the two-level block-Jacobi preconditioner (prealps_amd/csrc/coarse_space.c) is arithmetic on
a CSR panel: a stand-alone program (tests/c/coarse_space_check.c) links it alone, is compiled with
AddressSanitizer + UBSan and run as a program.  It builds zv, the chunk lists, E and Einv for cases written here;
SciPy and NumPy say what they should be.  The argument refusals of preAlps_BlockJacobiSetCoarseSpace that need no
GPU are checked through the library in plan-only mode."""
import ctypes as C
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
        pytest.fail("gcc is needed to build tests/c/coarse_space_check.c")
    tmp = tmp_path_factory.mktemp("coarse_space")
    out, unit = str(tmp / "coarse_space_check"), str(tmp / "coarse_space.o")
    flags = ["-O1", "-g", "-std=gnu11", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "coarse_space.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "coarse_space_check.c"), unit, "-o", out, "-lm"])
    return out, tmp


def permuted(A, part, nparts):
    """The matrix in the solver's internal order: rows grouped part by part, original order inside a part."""
    perm = np.argsort(part, kind="stable")
    B = sp.csr_matrix(A)[perm][:, perm].tocsr()
    B.sort_indices()
    rowpos = np.zeros(nparts + 1, dtype=np.int32)
    rowpos[1:] = np.cumsum(np.bincount(part, minlength=nparts))
    return B, rowpos, perm


def run_case(exe, name, A, rowpos, Vp, aggr=None, max_dofs=0, threads=0, omp=None):
    """One run of the program; returns a dict of everything it wrote."""
    prog, tmp = exe
    A = sp.csr_matrix(A)
    m, nparts, k = A.shape[0], len(rowpos) - 1, Vp.shape[1]
    naggr = 0 if aggr is None else int(np.max(aggr)) + 1
    fin, fout = str(tmp / (name + ".in")), str(tmp / (name + ".out"))
    with open(fin, "wb") as f:
        np.array([m, nparts, k, naggr, max_dofs, threads, A.nnz], dtype=np.int32).tofile(f)
        A.indptr.astype(np.int32).tofile(f)
        A.indices.astype(np.int32).tofile(f)
        A.data.astype(np.float64).tofile(f)
        np.asarray(rowpos, dtype=np.int32).tofile(f)
        if aggr is not None:
            np.asarray(aggr, dtype=np.int32).tofile(f)
        np.ascontiguousarray(Vp, dtype=np.float64).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    if omp is not None:
        env["OMP_NUM_THREADS"] = str(omp)
    run = subprocess.run([prog, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    raw = open(fout, "rb").read()
    o = {"raw": raw, "rc": int(np.frombuffer(raw, np.int32, 1)[0]), "msg": raw[4:260].split(b"\0")[0].decode()}
    h = np.frombuffer(raw, np.int32, 8, 260)
    o.update(nc=int(h[0]), naggr=int(h[1]), nchunks=int(h[2]), CH=int(h[3]), cap=int(h[4]), bad_aggr=int(h[5]), bad_vec=int(h[6]))
    off = 292
    o["part_aggregate"] = np.frombuffer(raw, np.int32, nparts, off); off += 4 * nparts
    if o["rc"] == 0:
        nch, nc = o["nchunks"], o["nc"]
        for key, n in (("ch_row0", nch), ("ch_nrows", nch), ("ch_aggr", nch), ("agg_ptr", o["naggr"] + 1), ("agg_chunk", nch)):
            o[key] = np.frombuffer(raw, np.int32, n, off); off += 4 * n
        o["zv"] = np.frombuffer(raw, np.float64, m * k, off).reshape(m, k); off += 8 * m * k
        o["E"] = np.frombuffer(raw, np.float64, nc * nc, off).reshape(nc, nc); off += 8 * nc * nc
        o["Einv"] = np.frombuffer(raw, np.float64, nc * nc, off).reshape(nc, nc); off += 8 * nc * nc
        assert off == len(raw)
    return o


def z_matrix(rowpos, aggr, Vp):
    m, k = Vp.shape
    g = np.repeat(np.asarray(aggr), np.diff(rowpos))
    rows = np.repeat(np.arange(m), k)
    cols = (g[:, None] * k + np.arange(k)[None, :]).ravel()
    return sp.csr_matrix((Vp.ravel(), (rows, cols)), shape=(m, (int(np.max(aggr)) + 1) * k))


def check_built(o, A, rowpos, aggr, Vp):
    m, k = Vp.shape
    aggr = np.asarray(aggr)
    assert o["rc"] == 0, o["msg"]
    assert o["nc"] == (aggr.max() + 1) * k
    assert np.array_equal(o["zv"], Vp)
    # chunks: every part cut into runs of at most CH consecutive rows, in order, with its aggregate
    want = [(r, min(o["CH"], rowpos[p + 1] - r), aggr[p]) for p in range(len(rowpos) - 1)
            for r in range(rowpos[p], rowpos[p + 1], o["CH"])]
    got = list(zip(o["ch_row0"], o["ch_nrows"], o["ch_aggr"]))
    assert got == [tuple(int(v) for v in w) for w in want]
    for g in range(o["naggr"]):
        lst = o["agg_chunk"][o["agg_ptr"][g]:o["agg_ptr"][g + 1]]
        assert np.array_equal(lst, np.flatnonzero(o["ch_aggr"] == g))       # ascending, complete
    Z = z_matrix(rowpos, aggr, Vp)
    Eref = (Z.T @ sp.csr_matrix(A) @ Z).toarray()
    # sums of at most (row length x rows of an aggregate) products: a rounding bound on |Z|^T |A| |Z|
    Eabs = (abs(Z).T @ abs(sp.csr_matrix(A)) @ abs(Z)).toarray()
    assert np.all(np.abs(o["E"] - Eref) <= 4 * m * EPS * Eabs + 1e-300)
    nc = o["nc"]
    cond = np.linalg.cond(Eref)
    assert np.abs(o["Einv"] @ Eref - np.eye(nc)).max() <= 100 * nc * EPS * cond
    assert np.array_equal(o["Einv"], o["Einv"].T)                          # symmetric in bits
    return cond


def poisson(n):
    from prealps_amd.gen import poisson3d_csr
    rp, ci, v = poisson3d_csr(n)
    return sp.csr_matrix((v, ci, rp), shape=(n ** 3, n ** 3))


def random_spd(n, seed, density=0.004):
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=density, random_state=np.random.RandomState(seed), format="csr")
    S = R + R.T
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 1.0 + rng.random(n)
    return (S + sp.diags(d)).tocsr()


def test_poisson_64_parts_constant_vector(exe):
    from prealps_amd.gen import box_partition
    A = poisson(12)
    part, nparts = box_partition(12, (3, 3, 3))
    assert nparts == 64
    B, rowpos, _ = permuted(A, part, nparts)
    Vp = np.ones((B.shape[0], 1))
    o = run_case(exe, "poisson64", B, rowpos, Vp, aggr=np.arange(64))
    cond = check_built(o, B, rowpos, np.arange(64), Vp)
    assert cond < 20                               # (cond E = 9.5 for this problem)
    # aggregates of several parts: four neighbouring boxes each
    aggr = np.arange(64) // 4
    o = run_case(exe, "poisson16", B, rowpos, Vp, aggr=aggr)
    check_built(o, B, rowpos, aggr, Vp)
    assert o["nc"] == 16


def test_random_spd_seven_parts_three_vectors(exe):
    A = random_spd(1500, 5)
    rowpos = np.array([0, 200, 430, 640, 860, 1070, 1290, 1500], dtype=np.int32)
    Vp = np.random.default_rng(6).standard_normal((1500, 3))
    o = run_case(exe, "random7", A, rowpos, Vp, aggr=np.arange(7))
    check_built(o, A, rowpos, np.arange(7), Vp)
    aggr = np.array([0, 0, 1, 1, 2, 2, 2])
    o = run_case(exe, "random3", A, rowpos, Vp, aggr=aggr)
    check_built(o, A, rowpos, aggr, Vp)


def test_one_row_part_and_part_longer_than_a_chunk(exe):
    A = random_spd(2900, 8, density=0.002)
    rowpos = np.array([0, 1, 2501, 2900], dtype=np.int32)           # 1 row, 2500 rows (three chunks), 399 rows
    Vp = np.random.default_rng(9).standard_normal((2900, 2))
    o = run_case(exe, "oddparts2", A, rowpos, Vp, aggr=np.arange(3))    # two vectors on one row are dependent
    assert o["rc"] == -4 and (o["bad_aggr"], o["bad_vec"]) == (0, 1)
    o = run_case(exe, "oddparts_joined", A, rowpos, Vp, aggr=np.array([0, 0, 1]))   # ... unless the part has company
    check_built(o, A, rowpos, np.array([0, 0, 1]), Vp)
    Vp = Vp[:, :1].copy()
    o = run_case(exe, "oddparts", A, rowpos, Vp, aggr=np.arange(3))
    check_built(o, A, rowpos, np.arange(3), Vp)
    assert o["CH"] < 2500 and o["nchunks"] == 1 + -(-2500 // o["CH"]) + 1
    assert 1 in o["ch_nrows"]


def test_same_bytes_for_one_and_eight_threads(exe):
    A = random_spd(1500, 5)
    rowpos = np.array([0, 200, 430, 640, 860, 1070, 1290, 1500], dtype=np.int32)
    Vp = np.random.default_rng(6).standard_normal((1500, 3))
    aggr = np.array([0, 0, 1, 1, 2, 3, 3])
    a = run_case(exe, "thr1", A, rowpos, Vp, aggr=aggr, omp=1)
    b = run_case(exe, "thr8", A, rowpos, Vp, aggr=aggr, omp=8)
    assert a["rc"] == 0 and a["raw"] == b["raw"]
    # the same through the unit's own argument, and on a coarse matrix large enough for its threaded loops
    from prealps_amd.gen import box_partition
    P = poisson(12)
    part, nparts = box_partition(12, (2, 2, 2))
    B, rp, _ = permuted(P, part, nparts)
    V1 = np.ones((B.shape[0], 1))
    a = run_case(exe, "p216t1", B, rp, V1, aggr=np.arange(nparts), threads=1)
    b = run_case(exe, "p216t8", B, rp, V1, aggr=np.arange(nparts), threads=8)
    assert a["rc"] == 0 and a["nc"] == 216 and a["raw"] == b["raw"]


def test_refusals(exe):
    A = random_spd(1500, 5)
    rowpos = np.array([0, 200, 430, 640, 860, 1070, 1290, 1500], dtype=np.int32)
    Vp = np.random.default_rng(6).standard_normal((1500, 3))
    o = run_case(exe, "cap", A, rowpos, Vp, aggr=np.arange(7), max_dofs=20)       # 21 unknowns
    assert o["rc"] == -2 and "cap is 20" in o["msg"]
    o = run_case(exe, "cap_ok", A, rowpos, Vp, aggr=np.arange(7), max_dofs=21)
    assert o["rc"] == 0
    o = run_case(exe, "empty", A, rowpos, Vp, aggr=np.array([0, 0, 1, 1, 3, 3, 3]))
    assert o["rc"] == -3 and "aggregate 2 is empty" in o["msg"]
    # the default cap is the unit's constant
    o = run_case(exe, "cap_default", A, rowpos, np.ones((1500, 8)), aggr=np.arange(7))
    assert o["cap"] >= 56 and o["rc"] == -4                                          # eight equal columns
    Vd = Vp.copy()
    Vd[:, 1] = Vd[:, 0]                                                              # a repeated column
    o = run_case(exe, "dependent", A, rowpos, Vd, aggr=np.arange(7))
    assert o["rc"] == -4 and (o["bad_aggr"], o["bad_vec"]) == (0, 1)
    assert "aggregate 0, vector 1" in o["msg"]
    Vz = Vp.copy()
    Vz[rowpos[4]:rowpos[5], 2] = 0.0                                                 # a vector that vanishes on a part
    o = run_case(exe, "vanishing", A, rowpos, Vz, aggr=np.arange(7))
    assert o["rc"] == -4 and (o["bad_aggr"], o["bad_vec"]) == (4, 2)


def test_default_aggregation_of_150_parts_at_a_small_cap(exe):
    from prealps_amd.gen import box_partition_nodes, elasticity3d_csr
    from prealps_amd.nearkernel import translations
    nn = (12, 10, 10)
    rp, ci, v = elasticity3d_csr(nn)
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    part, nparts = box_partition_nodes(nn, (2, 2, 2))
    assert nparts == 150
    B, rowpos, perm = permuted(A, part, nparts)
    Vp = translations(N, 3)[perm]
    o = run_case(exe, "default_small", B, rowpos, Vp, max_dofs=48)                  # 150 * 3 > 48: 16 aggregates
    assert o["rc"] == 0, o["msg"]
    assert o["naggr"] == 16 and o["nc"] == 48
    assert np.array_equal(o["part_aggregate"], np.arange(150) * 16 // 150)          # the program's partitioner: ranges
    check_built(o, B, rowpos, o["part_aggregate"], Vp)
    o = run_case(exe, "default_fits", B, rowpos, Vp, max_dofs=450)                  # one aggregate per part
    assert o["rc"] == 0 and o["naggr"] == 150 and np.array_equal(o["part_aggregate"], np.arange(150))


def test_near_kernel_vectors():
    from prealps_amd.gen import elasticity3d_csr
    from prealps_amd.nearkernel import rigid_body_modes, translations
    T = translations(12, 3)
    assert T.shape == (12, 3) and np.array_equal(T[:, 1], np.tile([0.0, 1.0, 0.0], 4))
    # rigid-body modes are in the kernel of the unconstrained Q1 stiffness: rows away from the fixed bottom layer
    nn = (4, 4, 5)
    rp, ci, v = elasticity3d_csr(nn, element="derived")
    N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    nid = np.arange(N // 3)
    coords = np.stack([nid % 4, (nid // 4) % 4, nid // 16], axis=1).astype(float)
    R = rigid_body_modes(coords)
    assert R.shape == (N, 6) and np.array_equal(R[:, :3], translations(N, 3))
    free = np.repeat(coords[:, 2] >= 2, 3)                                           # elements of the layers k >= 1 only
    assert np.abs((A @ R)[free]).max() <= 1e-12 * abs(A).max() * np.abs(R).max()


def test_library_refusals_in_plan_only_mode():
    import prealps_amd
    from prealps_amd.lib import PreAlpsError
    A = poisson(6)
    N = A.shape[0]
    prob = prealps_amd.EcgProblem(A.indptr, A.indices, A.data, 4, plan_only=True)
    try:
        L = prob.L
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
        cap = int(prob.stat("bj_coarse_max_dofs"))
        assert cap >= 8

        def refused(k, V, ldv, agg=None, naggr=0):
            rc = L.preAlps_BlockJacobiSetCoarseSpace(k, V.ctypes.data_as(pd) if V is not None else None, ldv,
                                                     agg.ctypes.data_as(pi) if agg is not None else None, naggr)
            assert rc != 0
            return L.preAlps_hip_last_error().decode()
        V = np.ones((N, 9), order="F")
        for k in (0, 9, -1):
            assert "k = %d" % k in refused(k, V, N)
        assert "V != NULL" in refused(1, None, N)
        assert "ldv = %d" % (N - 1) in refused(1, V, N - 1)
        Vn = V.copy(order="F")
        Vn[7, 1] = np.nan
        assert "V(7, 1) is not finite" in refused(2, Vn, N)
        Vn[7, 1] = np.inf
        assert "V(7, 1) is not finite" in refused(3, Vn, N)
        agg = np.zeros(4, dtype=np.int32)
        assert "the cap is %d" % cap in refused(2, V, N, agg, cap // 2 + 1)
        msg = refused(1, V, N)                          # well-formed: refused for the mode alone
        assert "plan-only" in msg and "preAlps_BlockJacobiSetCoarseSpace" in msg
        with pytest.raises(PreAlpsError, match="plan-only"):
            prob.set_coarse_space(V[:, :1])
        with pytest.raises(ValueError):
            prob.set_coarse_space(np.ones(N + 1))
        with pytest.raises(ValueError):
            prob.set_coarse_space(V[:, :1], aggregates=[0, 1])
        for key in ("bj_coarse_dofs", "bj_coarse_vectors", "bj_coarse_aggregates", "bj_coarse_chunks", "bj_coarse_bytes",
                    "bj_coarse_setup_s", "bj_coarse_builds", "bj_coarse_applies", "bj_coarse_einv_address"):
            assert prob.stat(key) == 0
        assert L.preAlps_BlockJacobiClearCoarseSpace() == 0
    finally:
        prob.close()
