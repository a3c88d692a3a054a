"""Every BASELINE.json configuration exercised through the C ABI against the CPU oracle at a size
the oracle finishes in seconds (the matrix class, enlarging factor, variant and reduction of the
configuration; the size is what shrinks), plus the full-size headline workload's first
iterations, the dispatch paths of the block solve that small problems would not reach, and the
BF-Omin shrink.  fp64; residual histories to 1e-8 relative unless a test says otherwise."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL_HIST = 1e-8


def _problem(A, P, part=None, **kw):
    import prealps_amd
    from oracle import oracle as O
    part = O.contiguous_partition(A.shape[0], P) if part is None else part
    rp, ci, v = O.as_csr(A)
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0, **kw)
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
    return prob, B, rowpos


def _elasticity(nn, box):
    from prealps_amd import gen
    rp, ci, v = gen.elasticity3d_csr(nn)
    part, nparts = gen.box_partition_nodes(nn, box)
    N = len(rp) - 1
    return sp.csr_matrix((v, ci, rp), shape=(N, N)), part, nparts


def _algs(name):
    import prealps_amd as pa
    from oracle import oracle as O
    return {"odir": (pa.ORTHODIR, O.ORTHODIR), "omin": (pa.ORTHOMIN, O.ORTHOMIN),
            "fused": (pa.ORTHODIR_FUSED, O.ORTHODIR_FUSED)}[name]


# ---- configs[0]: elasticity3d 12 x 10 x 10, ECG + block-Jacobi, t = 4, 8 subdomains ------------------
def test_config0_elasticity_12x10x10_t4_p8():
    """`test_ecg_prealps_op -e 4 -o 0 -r 0` on the stand-in for matrix/elasticity3d_12x10x10_var.mtx
    (SURVEY 8d C1(iii)): the reference's element matrix on 12 x 10 x 10 nodes, 8 subdomains from
    the graph partitioner (the reference: METIS), tol 1e-5, at most 1000 iterations."""
    import prealps_amd as pa
    from prealps_amd import gen
    from prealps_amd.solver import partition_kway
    from oracle import oracle as O
    rp, ci, v = gen.elasticity3d_csr((12, 10, 10))
    N = 3600
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    part = partition_kway(rp, ci, 8)
    prob, B, rowpos = _problem(A, 8, part)
    try:
        rhs = prob.reference_rhs()
        np.testing.assert_array_equal(rhs, O.reference_rhs(rowpos))
        got = prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, bs_red=pa.NO_BS_RED, tol=1e-5, max_iter=1000)
        ref = O.ECG(B, rowpos, 4, O.ORTHODIR, O.NO_BS_RED, 1e-5, 1000).solve(rhs)
        # Coefficient jumps of 1e10: two fp64 implementations of the same recurrence drift apart
        # exponentially (tools/history_probe.py -> profiles/r03_history_divergence.txt: 1e-13 after the
        # first iteration, a factor ~10 every 10 iterations; this case converges in 31 iterations with
        # the library's partition, by when the drift has reached 1e-7).  Two CPU paths -- the oracle and
        # the reference's MKL kernels -- separate the same way (tools/history_control.py,
        # tests/test_history_control_cpu.py), so it is the recurrence, not the HIP path.  Hence: the
        # first 20 residuals to 1e-8, the rest to 1e-4, the iteration count within 3, and both answers
        # solve the system.
        k = min(len(got.res), len(ref["res"]))
        np.testing.assert_allclose(got.res[:20], ref["res"][:20], rtol=RTOL_HIST)
        np.testing.assert_allclose(got.res[:k - 3], ref["res"][:k - 3], rtol=1e-4)
        assert abs(got.iters - ref["iters"]) <= 3 and got.iters < 1000
        assert got.final_res <= 1e-5 * got.normb
        for x, res in ((got.x, got.final_res), (ref["x"], ref["final_res"])):
            assert np.linalg.norm(rhs - B @ x) <= 4.0 * res + 1e-12    # (true vs recurrence residual: they part ways on this matrix)
    finally:
        prob.close()


# ---- configs[2]: an unstructured SPD matrix (Flan_1565's class), t = 4, through the partitioner -----
def _unstructured_spd(npts, seed):
    """Graph Laplacian + mass of a random point cloud in the unit cube (12 nearest neighbours,
    3 dofs per point coupled by a random SPD 3 x 3 block), randomly renumbered: no grid, no
    geometry in the ids, vector-valued like a 3-D mechanics matrix."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    X = rng.random((npts, 3))
    _, nb = cKDTree(X).query(X, k=13)
    rows = np.repeat(np.arange(npts), 12)
    cols = nb[:, 1:].ravel()
    G = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(npts, npts)).tocsr()
    G = ((G + G.T) > 0).astype(np.float64)                    # symmetric pattern
    W = sp.triu(G, 1).tocoo()
    w = 0.5 + rng.random(W.nnz)                                # edge stiffness
    K = rng.standard_normal((W.nnz, 3, 3))
    K = np.einsum("eij,ekj->eik", K, K) + 0.2 * np.eye(3)     # SPD 3 x 3 per edge
    K *= w[:, None, None]
    n3 = 3 * npts
    i3 = (3 * W.row[:, None, None] + np.arange(3)[None, :, None]) + 0 * np.arange(3)[None, None, :]
    j3 = (3 * W.col[:, None, None] + np.arange(3)[None, None, :]) + 0 * np.arange(3)[None, :, None]
    ii = (3 * W.row[:, None, None] + np.arange(3)[None, :, None]) + 0 * np.arange(3)[None, None, :]
    jj = (3 * W.row[:, None, None] + np.arange(3)[None, None, :]) + 0 * np.arange(3)[None, :, None]
    kk = (3 * W.col[:, None, None] + np.arange(3)[None, :, None]) + 0 * np.arange(3)[None, None, :]
    ll = (3 * W.col[:, None, None] + np.arange(3)[None, None, :]) + 0 * np.arange(3)[None, :, None]
    A = (sp.coo_matrix((-K.ravel(), (i3.ravel(), j3.ravel())), shape=(n3, n3)) +
         sp.coo_matrix((-np.transpose(K, (0, 2, 1)).ravel(), (j3.transpose(0, 2, 1).ravel(), i3.transpose(0, 2, 1).ravel())), shape=(n3, n3)) +
         sp.coo_matrix((K.ravel(), (ii.ravel(), jj.ravel())), shape=(n3, n3)) +
         sp.coo_matrix((K.ravel(), (kk.ravel(), ll.ravel())), shape=(n3, n3))).tocsr()
    A = A + 0.05 * sp.identity(n3)
    A = 0.5 * (A + A.T)
    q = rng.permutation(npts)
    q3 = (3 * q[:, None] + np.arange(3)[None, :]).ravel()
    A = sp.csr_matrix(A[q3][:, q3])
    A.sum_duplicates()
    A.sort_indices()
    return A


def test_config2_unstructured_matrix_through_the_partitioner(tmp_path):
    """BASELINE configs[2] (Flan_1565: unstructured 3-D mechanics, t = 4): no such file offline, so
    an unstructured vector-valued SPD matrix is generated, written as MatrixMarket and solved
    through preAlps_OperatorBuild -- reader, scaling, the library's graph partitioner where the
    reference calls METIS, permutation -- exactly like the reference driver; the oracle gets the
    same partition.  The same matrix in memory with the explicit partition must agree too."""
    import scipy.io
    import prealps_amd as pa
    from oracle import oracle as O
    A = _unstructured_spd(2500, 4)
    N, P, t = A.shape[0], 40, 4
    path = str(tmp_path / "unstructured.mtx")
    scipy.io.mmwrite(path, sp.tril(A), symmetry="symmetric")
    prob = pa.EcgProblem.from_mtx(path, nparts=P)
    try:
        part = prob.part_vector()
        sizes = np.bincount(part, minlength=P)
        assert sizes.min() > 0 and sizes.max() <= 1.25 * N / P
        A2 = O.load_mtx(path)
        B, perm, rowpos = O.permute_by_part(O.symrac_scale(A2), part, P)
        np.testing.assert_array_equal(prob.rowpos, rowpos)
        rhs = prob.reference_rhs()
        np.testing.assert_array_equal(rhs, O.reference_rhs(rowpos))
        got = prob.solve(rhs, t, max_iter=1000)
        ref = O.ECG(B, rowpos, t, max_iter=1000).solve(rhs)
        assert got.iters == ref["iters"] and got.iters < 1000
        np.testing.assert_allclose(got.res, ref["res"], rtol=1e-7)
        np.testing.assert_allclose(got.x, ref["x"], rtol=1e-6, atol=1e-8 * np.abs(ref["x"]).max())
        band_kway = prob.stat("bj_max_bandwidth")
    finally:
        prob.close()
    # the same through the in-memory builder with the partition handed over explicitly
    prob2, B2, rowpos2 = _problem(A2, P, part)
    try:
        got2 = prob2.solve(prob2.reference_rhs(), t, max_iter=1000)
        assert got2.iters == got.iters
        np.testing.assert_allclose(got2.res, got.res, rtol=1e-9)
    finally:
        prob2.close()
    # contiguous row blocks of the randomly numbered matrix are not subdomains at all (their
    # diagonal blocks are nearly diagonal): the partitioner's parts converge much faster
    prob3, B3, rowpos3 = _problem(A2, P, None)
    try:
        got3 = prob3.solve(prob3.reference_rhs(), t, max_iter=1000)
        assert got3.iters > 1.3 * got.iters and band_kway > prob3.stat("bj_max_bandwidth")
    finally:
        prob3.close()


# ---- configs[3]: elasticity, t = 8, Odir / Omin with dynamic reduction of the search directions ------
@pytest.mark.parametrize("alg", ["odir", "omin", "fused"])
def test_config3_elasticity_t8_with_block_size_reduction(alg):
    """`-e 8 -o {0,1} -r 1`: D-Odir (SVD threshold + rotation, ecg.c:445-497) and BF-Omin (pivoted
    Cholesky, ecg.c:361-393) on the elasticity matrix class: residuals AND block size sequence."""
    import prealps_amd as pa
    from oracle import oracle as O
    A, part, nparts = _elasticity(9, (3, 3, 3))
    prob, B, rowpos = _problem(A, nparts, part)
    try:
        a_gpu, a_cpu = _algs(alg)
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, 8, ortho_alg=a_gpu, bs_red=pa.ADAPT_BS, max_iter=600)
        ref = O.ECG(B, rowpos, 8, a_cpu, O.ADAPT_BS, 1e-5, 600).solve(rhs)
        assert got.iters == ref["iters"]
        assert list(got.bs) == list(ref["bs"])
        np.testing.assert_allclose(got.res, ref["res"], rtol=1e-6)
        if alg == "odir":
            assert got.bs[-1] < 8          # the reduction really happened
    finally:
        prob.close()


_RCI_REDUCTION_SNIPPET = r"""
import sys, os
sys.path.insert(0, %r)
import ctypes as C
import numpy as np, scipy.sparse as sp
import prealps_amd as pa
import prealps_amd.lib as pl
from prealps_amd import gen
from prealps_amd.lib import check
from oracle import oracle as O
rp, ci, v = gen.elasticity3d_csr(9)
part, P = gen.box_partition_nodes(9, (3, 3, 3))
A = sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))
B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
rhs = prob.reference_rhs()
L = prob.L
for alg_g, alg_o in ((pl.ORTHODIR, O.ORTHODIR), (pl.ORTHOMIN, O.ORTHOMIN)):
    ref = O.ECG(B, rowpos, 8, alg_o, O.ADAPT_BS, 1e-5, 600).solve(rhs)
    own = prob.solve(rhs, 8, ortho_alg=alg_g, bs_red=pl.ADAPT_BS, max_iter=600)
    e = prob.new_ecg(8, alg_g, pl.ADAPT_BS, 1e-5, 600)
    rci, stop = C.c_int(0), C.c_int(0)
    check(L.preAlps_ECGInitialize(C.byref(e), rhs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rci)), "init")
    check(L.preAlps_BlockJacobiApply(e.R, e.P), "bj")
    hist, bs = [], []
    while stop.value != 1:               # examples/test_ecg_prealps_op.c:203-223
        if rci.value == 0:
            check(L.preAlps_BlockOperator(e.P, e.AP), "op")
        else:
            check(L.preAlps_ECGStoppingCriterion(C.byref(e), C.byref(stop)), "stop")
            hist.append(e.res); bs.append(e.bs)
            if stop.value == 1: break
            check(L.preAlps_BlockJacobiApply(e.R if alg_g == pl.ORTHOMIN else e.AP, e.Z), "bj")
        check(L.preAlps_ECGIterate(C.byref(e), C.byref(rci)), "iterate")
    sol = (C.c_double * prob.m)()
    check(L.preAlps_ECGFinalize(C.byref(e), sol), "fin")
    assert len(hist) == ref["iters"] == own.iters, (len(hist), ref["iters"], own.iters)
    assert bs == list(ref["bs"]) == list(own.bs), (bs, list(ref["bs"]))
    if alg_g == pl.ORTHODIR: assert bs[-1] < 8 and bs[0] == 8
    np.testing.assert_allclose(hist, ref["res"], rtol=1e-6)
    np.testing.assert_allclose(hist, own.res, rtol=1e-6)
    np.testing.assert_allclose(np.asarray(sol[:]), ref["x"], rtol=1e-5, atol=1e-7 * np.abs(ref["x"]).max())
prob.close()
print("rci reduction ok")
"""


@pytest.mark.parametrize("knob", ["PREALPS_ECG_LAZY_NORM=1", "PREALPS_ECG_LAZY_NORM=0", "PREALPS_ECG_FUSE=0"])
def test_block_size_reduction_through_the_callers_own_loop(knob):
    """D-Odir and BF-Omin at 8 columns driven by the caller (the loop of examples/test_ecg_prealps_op.c:203-223,
    every step a separate call): residuals, block-size sequence and solution against the oracle and against the
    library's own loop.  While every direction is live D-Odir keeps its panels un-normalised (ecg.c `lazy_norm`),
    in the library's loop it also queues the block solve before the host looks at alpha; the first reduction writes
    the normalised panels and goes on in the reference's order.  PREALPS_ECG_LAZY_NORM=0: normalised throughout;
    PREALPS_ECG_FUSE=0: the reference's four passes, BF-Omin's copy / permutation / solve as three kernels."""
    env = dict(os.environ, **dict([knob.split("=")]))
    r = subprocess.run([sys.executable, "-c", _RCI_REDUCTION_SNIPPET % ROOT], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "rci reduction ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])


@pytest.mark.parametrize("alg", ["odir", "omin"])
def test_config3_elasticity_t8_no_reduction(alg):
    import prealps_amd as pa
    from oracle import oracle as O
    A, part, nparts = _elasticity(9, (3, 3, 3))
    prob, B, rowpos = _problem(A, nparts, part)
    try:
        a_gpu, a_cpu = _algs(alg)
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, 8, ortho_alg=a_gpu, max_iter=600)
        ref = O.ECG(B, rowpos, 8, a_cpu, O.NO_BS_RED, 1e-5, 600).solve(rhs)
        assert got.iters == ref["iters"]
        np.testing.assert_allclose(got.res, ref["res"], rtol=1e-6)
        np.testing.assert_allclose(got.x, ref["x"], rtol=1e-5, atol=1e-8 * np.abs(ref["x"]).max())
    finally:
        prob.close()


# ---- configs[4]: the large elasticity-class matrix, t = 16 ------------------------------------------------
def test_config4_elasticity_t16_odir():
    import prealps_amd as pa
    from oracle import oracle as O
    A, part, nparts = _elasticity(10, (2, 4, 5))      # 5 x 3 x 2 = 30 subdomains >= t
    prob, B, rowpos = _problem(A, nparts, part)
    try:
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, 16, max_iter=400)
        ref = O.ECG(B, rowpos, 16, O.ORTHODIR, O.NO_BS_RED, 1e-5, 400).solve(rhs)
        assert got.iters == ref["iters"]
        np.testing.assert_allclose(got.res, ref["res"], rtol=1e-6)
        np.testing.assert_allclose(got.x, ref["x"], rtol=1e-5, atol=1e-8 * np.abs(ref["x"]).max())
    finally:
        prob.close()


def test_unstructured_matrix_at_sixteen_columns():
    """BASELINE configs[4]'s class (Queen_4147: unstructured, t = 16) at a size the oracle solves: the
    unstructured 3-dof SPD matrix of the configs[2] test through the library's partitioner with 16 search
    directions -- the 16-column SpMM (two 8-column halves of the run plan, or L2 gathers where rows do not
    come in runs), the matrix-core Gram / update / trsm kernels and the 16-column block solve."""
    import prealps_amd as pa
    from prealps_amd.solver import partition_kway
    from oracle import oracle as O
    A = _unstructured_spd(3000, 9)
    N, P, t = A.shape[0], 48, 16
    A = sp.csr_matrix(A)
    A.sort_indices()
    part = partition_kway(A.indptr.astype(np.int32), A.indices.astype(np.int32), P)
    prob, B, rowpos = _problem(A, P, part)
    try:
        X = np.random.default_rng(16).standard_normal((N, t))
        ref = O.spmm(B, X)
        np.testing.assert_allclose(prob.block_operator(X, t), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        zr = O.BlockJacobi(B, rowpos).apply(X)
        np.testing.assert_allclose(prob.block_jacobi_apply(X, t), zr, rtol=1e-9, atol=1e-10 * np.abs(zr).max())
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, t, max_iter=1000)
        refs = O.ECG(B, rowpos, t, max_iter=1000).solve(rhs)
        assert got.iters == refs["iters"] and got.iters < 1000
        np.testing.assert_allclose(got.res, refs["res"], rtol=1e-7)
        np.testing.assert_allclose(got.x, refs["x"], rtol=1e-6, atol=1e-8 * np.abs(refs["x"]).max())
    finally:
        prob.close()


# ---- the headline workload at full size: first iterations against the oracle -----------------------------
@pytest.mark.parametrize("factor", ["device", "host"])
def test_full_size_first_residuals_vs_oracle(factor, monkeypatch):
    """Q1 elasticity 70^3 nodes (N = 1,029,000, nnz = 80,990,208), t = 4, 5670 subdomains of
    2 x 4 x 8 nodes -- the bench default.  The oracle runs 16 iterations of the same problem on the
    host cores; the residual norm after every one of them must agree to 1e-8 (observed: 1e-11),
    with the block factors computed on the device and on the host."""
    monkeypatch.setenv("PREALPS_BJ_FACTOR", factor)
    import prealps_amd as pa
    from oracle import oracle as O
    A, part, nparts = _elasticity(70, (2, 4, 8))
    prob, B, rowpos = _problem(A, nparts, part)
    try:
        assert B.nnz == 80990208 and nparts == 5670
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, 4, max_iter=16)
        ref = O.ECG(B, rowpos, 4, O.ORTHODIR, O.NO_BS_RED, 1e-5, 16).solve(rhs)
        assert len(got.res) == len(ref["res"]) == 16
        assert abs(got.normb - ref["normb"]) <= 1e-13 * ref["normb"]
        np.testing.assert_allclose(got.res, ref["res"], rtol=RTOL_HIST)
    finally:
        prob.close()


# ---- dispatch paths of the block solve ---------------------------------------------------------------------
@pytest.mark.parametrize("wide_from", ["default", "448"])
@pytest.mark.parametrize("n,t,lo,hi", [(8, 8, 49, 80), (8, 16, 49, 80), (11, 8, 81, 112), (11, 16, 81, 112), (11, 4, 81, 112),
                                       (14, 4, 129, 192), (16, 4, 193, 256), (20, 4, 257, 320), (22, 4, 321, 384),
                                       (24, 2, 385, 448), (20, 8, 257, 320)])
def test_block_solve_dispatch_by_band(n, t, lo, hi, wide_from, monkeypatch):
    """Two cubes of n^3 Poisson nodes -> band ~0.8 n^2 after reordering: 49..80 (matrix cores, 6
    tiles at 8 / 16 columns), 81..112 (8 tiles, 64 KiB of LDS), then the register-set classes
    R = 4, 5, 6, 7, 8 of the one-wavefront kernel (bands up to 448).  With fewer than 1024 blocks
    the library sends bands above 96 to the workgroup-per-block kernel; PREALPS_BJ_WIDE_FROM=448
    forces the wavefront-per-block kernels that production sizes (>= 1024 blocks per GPU) use.
    Both against the oracle's solve."""
    if wide_from != "default":
        monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", wide_from)
    monkeypatch.setenv("PREALPS_BJ_ND", "0")      # (blocks this large would otherwise get the sparse factor: tested below)
    from oracle import oracle as O
    import scipy.sparse as sp2
    T = sp2.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    T2 = sp2.diags([-np.ones(2 * n - 1), 2 * np.ones(2 * n), -np.ones(2 * n - 1)], [-1, 0, 1])
    I, I2 = sp2.identity(n), sp2.identity(2 * n)
    A = sp.csr_matrix(sp2.kron(sp2.kron(T2, I), I) + sp2.kron(sp2.kron(I2, T), I) + sp2.kron(sp2.kron(I2, I), T))
    prob, B, rowpos = _problem(A, 2)
    try:
        X = np.random.default_rng(n + t).standard_normal((B.shape[0], t))
        zr = O.BlockJacobi(B, rowpos).apply(X)
        got = prob.block_jacobi_apply(X, t)
        np.testing.assert_allclose(got, zr, rtol=1e-9, atol=1e-10 * np.abs(zr).max())
        assert lo <= prob.stat("bj_max_bandwidth") <= hi, prob.stat("bj_max_bandwidth")
    finally:
        prob.close()


# ---- the one-copy matrix-core band solve (bj_g4.hip) and the kernels it replaced ---------------------------
def _boxes_problem(n, box, t, seed):
    from prealps_amd import gen
    rp, ci, v = gen.poisson3d_csr(n)
    part, P = gen.box_partition(n, box)
    A = sp.csr_matrix((v, ci, rp), shape=(n ** 3, n ** 3))
    prob, B, rowpos = _problem(A, P, part)
    X = np.random.default_rng(seed).standard_normal((n ** 3, t))
    return prob, B, rowpos, X


@pytest.mark.parametrize("g4", ["1", "0"])
@pytest.mark.parametrize("n,box,t", [(20, (5, 5, 10), 4), (24, (4, 4, 12), 4), (12, (6, 6, 6), 4), (24, (6, 4, 8), 3),
                                     (24, (8, 3, 8), 2), (24, (8, 8, 3), 1), (21, (7, 7, 3), 4), (20, (5, 5, 2), 4),
                                     (18, (9, 9, 3), 4), (20, (10, 10, 2), 4)])
def test_band_solve_for_up_to_four_columns(n, box, t, g4, monkeypatch):
    """Panels of up to 4 columns on blocks of up to 256 rows with bands up to 112: ONE copy of the band for
    both sweeps on the f64 matrix cores (bj_g4.hip: 12 / 14 / 16 register tiles, 3 .. 8 tiles under a group's
    record; blocks that fill their last tile, rows that are no multiple of 4 or 8, panel strides 2 and 4,
    fewer columns than the stride) -- and, with PREALPS_BJ_G4=0, the register recurrence on two copies that
    it replaced (k_bj_apply_pairs / k_bj_apply).  Both against the oracle's exact block solve."""
    monkeypatch.setenv("PREALPS_BJ_G4", g4)
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    from oracle import oracle as O
    prob, B, rowpos, X = _boxes_problem(n, box, t, n + t)
    try:
        zr = O.BlockJacobi(B, rowpos).apply(X)
        got = prob.block_jacobi_apply(X, t)
        np.testing.assert_allclose(got, zr, rtol=1e-11, atol=1e-12 * np.abs(zr).max())
        assert (prob.stat("bj_g4_bytes") > 0) == (g4 == "1")
        # several applies in a row give the same bits (no race between the prefetch ring and the sweeps)
        again = prob.block_jacobi_apply(X, t)
        np.testing.assert_array_equal(got, again)
    finally:
        prob.close()


@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("n,box,t", [(20, (5, 5, 10), 8), (24, (4, 4, 12), 8), (12, (6, 6, 6), 7), (24, (8, 3, 8), 5), (24, (6, 4, 8), 6),
                                     (24, (4, 4, 12), 16), (16, (4, 4, 8), 16), (16, (4, 4, 4), 12), (16, (4, 4, 8), 8)])
def test_band_solve_for_eight_columns(n, box, t, wide, monkeypatch):
    """Panels of 5 .. 8 columns: two column sets per wavefront on the one-copy records (bj_g4.hip, bands up to
    80) and, with PREALPS_BJ_G4_WIDE=0, the two-copy matrix-core kernel k_bj_mfma it stands in for; panels of 9 ..
    16 columns always run k_bj_mfma.  Blocks of 64 / 128 / 192 rows fill their last tile of 16 rows exactly: the
    case in which bj_g4.hip's hand-issued lane moves once read a matrix-instruction result too early (run-to-run
    different bits) -- k_bj_mfma's moves go through the compiler's hazard recogniser now; repeated applies must
    give the same bits."""
    monkeypatch.setenv("PREALPS_BJ_G4_WIDE", wide)
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    from oracle import oracle as O
    prob, B, rowpos, X = _boxes_problem(n, box, t, n + t)
    try:
        zr = O.BlockJacobi(B, rowpos).apply(X)
        got = prob.block_jacobi_apply(X, t)
        np.testing.assert_allclose(got, zr, rtol=1e-11, atol=1e-12 * np.abs(zr).max())
        for _ in range(3):
            np.testing.assert_array_equal(got, prob.block_jacobi_apply(X, t))
    finally:
        prob.close()


@pytest.mark.parametrize("ring", ["2", "4", "8"])
def test_band_solve_prefetch_ring_depths(ring, monkeypatch):
    """The prefetch ring of bj_g4.hip at every depth (few blocks get 8 buffers by default, many get 2)."""
    monkeypatch.setenv("PREALPS_BJ_G4_RING", ring)
    from oracle import oracle as O
    for n, box in ((20, (5, 5, 10)), (24, (4, 4, 12)), (16, (4, 4, 8))):
        prob, B, rowpos, X = _boxes_problem(n, box, 4, 7)
        try:
            zr = O.BlockJacobi(B, rowpos).apply(X)
            np.testing.assert_allclose(prob.block_jacobi_apply(X, 4), zr, rtol=1e-11, atol=1e-12 * np.abs(zr).max())
        finally:
            prob.close()


# ---- large blocks: sparse (nested dissection) factor against the band factor and the oracle -----------
@pytest.mark.parametrize("variant", ["device", "host", "chains"])
@pytest.mark.parametrize("t", [1, 4, 8, 16])
@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_large_blocks_sparse_factor(kind, t, variant, monkeypatch):
    """Few large subdomains (nparts = 64 on 1M rows, the reference's one block per
    rank): blocks of >= 2048 rows with a wide band get the supernodal factor of nd.c in
    selective-inversion form, solved level by level (k_nd_forward / k_nd_backward).  Same answer
    as the oracle's exact block solve and as the band kernels (PREALPS_BJ_ND=0) on the same
    blocks -- with the numeric phase on the device (nd_factor.hip, the default), on the host
    threads, and with separators cut into chains of 64-column supernodes over small leaves."""
    from oracle import oracle as O
    if variant == "host":
        monkeypatch.setenv("PREALPS_ND_NUMERIC", "host")
    if variant == "chains":
        monkeypatch.setenv("PREALPS_ND_WIDTH", "64")
        monkeypatch.setenv("PREALPS_ND_LEAF", "24")
    if kind == "poisson":
        A, P, part = O.poisson3d(24), 2, None          # slabs of 12 x 24 x 24 = 6912 rows, band 288
    else:
        A, part, P = _elasticity(14, (14, 14, 7))      # 2 blocks of 14 x 14 x 7 nodes = 4116 rows, band ~300
    X = np.random.default_rng(t).standard_normal((A.shape[0], t))
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PREALPS_BJ_ND", mode)
        prob, B, rowpos = _problem(A, P, part)
        try:
            out[mode] = prob.block_jacobi_apply(X, t)
            assert prob.stat("bj_nd_blocks") == (P if mode == "1" else 0)
            if mode == "1":
                nd_bytes = prob.stat("bj_factor_bytes")
                # the inverted pivot triangles, checked where they were made (device: k_ndf_check)
                assert 0.0 < prob.stat("bj_nd_inverse_dev") < 1e-10
            else:
                assert nd_bytes < prob.stat("bj_factor_bytes")          # the sparse factor is the smaller one
        finally:
            prob.close()
    zr = O.BlockJacobi(B, rowpos).apply(X)
    tol = 1e-9 if kind == "poisson" else 1e-7       # (coefficient jumps of 1e10 in the elasticity blocks)
    for mode in out:
        np.testing.assert_allclose(out[mode], zr, rtol=tol, atol=tol * np.abs(zr).max())


def test_large_blocks_that_are_no_grids(monkeypatch):
    """The sparse factor (ordering, device factorisation, selective inversion, level-scheduled
    solve) on blocks without geometry: a random pattern (expander-like, separators of hundreds of
    columns -> chains of supernodes), nearest-neighbour links of random points in a cube, and a block
    made of two disconnected halves; against the oracle's exact block solve and in a full ECG solve."""
    from oracle import oracle as O
    from scipy.spatial import cKDTree
    monkeypatch.setenv("PREALPS_BJ_ND", "2")
    nb, P, t = 2600, 4, 4
    rng = np.random.default_rng(7)
    blocks = []
    for p in range(P):
        if p == 2:
            h = nb // 2
            M = sp.block_diag([sp.random(h, h, density=6.0 / h, random_state=rng),
                               sp.random(nb - h, nb - h, density=14.0 / nb, random_state=rng)], format="csr")
        elif p == 1:
            pts = rng.random((nb, 3))
            _, idx = cKDTree(pts).query(pts, k=9)
            M = sp.csr_matrix((rng.random(8 * nb), (np.repeat(np.arange(nb), 8), idx[:, 1:].ravel())), shape=(nb, nb))
        else:
            M = sp.random(nb, nb, density=5.0 / nb, random_state=rng, format="csr")
        blocks.append(M + M.T)
    A = sp.lil_matrix(sp.block_diag(blocks))
    for _ in range(100):                       # a few couplings between the blocks
        i, j = rng.integers(0, nb * P, 2)
        A[i, j] = A[j, i] = 0.1
    A = sp.csr_matrix(A)
    A = sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.5))
    A.sort_indices()
    part = (np.arange(nb * P) // nb).astype(np.int32)
    prob, B, rowpos = _problem(A, P, part)
    try:
        X = rng.standard_normal((B.shape[0], t))
        zr = O.BlockJacobi(B, rowpos).apply(X)
        got = prob.block_jacobi_apply(X, t)
        assert prob.stat("bj_nd_blocks") == P and prob.stat("bj_nd_inverse_dev") < 1e-11
        np.testing.assert_allclose(got, zr, rtol=1e-10, atol=1e-11 * np.abs(zr).max())
        rhs = prob.reference_rhs()
        res = prob.solve(rhs, t)
        ref = O.ECG(B, rowpos, t).solve(rhs)
        assert res.iters == ref["iters"]
        np.testing.assert_allclose(res.res, ref["res"], rtol=1e-7)
    finally:
        prob.close()


def test_mtx_file_with_every_default(tmp_path):
    """The reference driver's path with nothing chosen by hand: a MatrixMarket file, the library's
    partitioner (8 parts of 8000 rows, band ~340), which are large enough for the sparse factor, factored on the
    device -- the same iterations and residuals as the oracle on the partition the library made."""
    import scipy.io
    import prealps_amd as pa
    from oracle import oracle as O
    n = 40
    A = O.poisson3d(n)
    f = str(tmp_path / "p40.mtx")
    scipy.io.mmwrite(f, sp.tril(A), symmetry="symmetric")
    prob = pa.EcgProblem.from_mtx(f, 8)
    try:
        prob.create_block_jacobi()
        assert prob.stat("bj_nd_blocks") == 8 and prob.stat("bj_nd_inverse_dev") < 1e-11
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, 4)
        part = prob.part_vector()
        B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, 8)
        ref = O.ECG(B, rowpos, 4).solve(O.reference_rhs(rowpos))
        assert got.iters == ref["iters"]
        np.testing.assert_allclose(got.res, ref["res"], rtol=1e-8)
    finally:
        prob.close()


def test_large_blocks_ecg_and_mixed_sizes(monkeypatch):
    """ECG on a partition that mixes one large block (sparse factor) with many small ones (band
    kernels), every leaf size of the dissection, and a non-SPD large block reported as such."""
    import prealps_amd as pa
    from oracle import oracle as O
    n = 20
    A = O.poisson3d(n)
    idx = np.arange(n ** 3)
    i = idx // (n * n)
    part = np.where(i < 14, 0, 1 + (idx - 14 * n * n) // 200).astype(np.int32)      # 5600 rows (band 280), then blocks of 200
    P = int(part.max()) + 1
    monkeypatch.setenv("PREALPS_ND_LEAF", "40")
    monkeypatch.setenv("PREALPS_BJ_ND", "2")
    prob, B, rowpos = _problem(A, P, part)
    try:
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, 4)
        assert prob.stat("bj_nd_blocks") == 1
        ref = O.ECG(B, rowpos, 4).solve(rhs)
        assert got.iters == ref["iters"]
        np.testing.assert_allclose(got.res, ref["res"], rtol=RTOL_HIST)
    finally:
        prob.close()
    Ab = sp.lil_matrix(A)
    Ab[777, 777] = -5.0
    prob, B, rowpos = _problem(sp.csr_matrix(Ab), P, part)
    try:
        with pytest.raises(pa.PreAlpsError, match="not SPD"):
            prob.create_block_jacobi()
    finally:
        prob.close()


# ---- BF-Omin really shrinks ------------------------------------------------------------------------------------
def test_bf_omin_shrinks_when_a_direction_dies():
    """Breakdown-free Orthomin (ecg.c:361-393): subdomains 3, 7, 11, ... (p mod 4 == 3) are cut off
    from the rest of the matrix.  Column 3 of the split residual lives on exactly those rows, the
    block-Jacobi solve is exact for them, so that column converges in one iteration, its search
    direction degenerates to rounding noise and the pivoted Cholesky of P^T P finds rank 3: the
    block size must drop from 4 to 3 in the reference algorithm and here, at the same iteration."""
    import prealps_amd as pa
    from oracle import oracle as O
    n, P, t = 16, 16, 4
    # (a random diagonal: on the plain Laplacian the mirror symmetry of the slabs kills a second
    # direction too, and which of two rounding-level pivots survives is not a property to pin)
    A = O.poisson3d(n) + sp.diags(np.random.default_rng(1).random(n ** 3))
    part = O.contiguous_partition(n ** 3, P)
    coo = sp.coo_matrix(A)
    cutoff = (part[coo.row] != part[coo.col]) & ((part[coo.row] % t == t - 1) | (part[coo.col] % t == t - 1))
    A = sp.csr_matrix((coo.data[~cutoff], (coo.row[~cutoff], coo.col[~cutoff])), shape=coo.shape)
    prob, B, rowpos = _problem(A, P, part)
    try:
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, t, ortho_alg=pa.ORTHOMIN, bs_red=pa.ADAPT_BS, max_iter=300)
        ref = O.ECG(B, rowpos, t, O.ORTHOMIN, O.ADAPT_BS, 1e-5, 300).solve(rhs)
        assert list(ref["bs"][:3]) == [4, 3, 3], "the construction did not make the oracle shrink by one"
        assert list(got.bs) == list(ref["bs"])
        assert got.iters == ref["iters"]
        np.testing.assert_allclose(got.res, ref["res"], rtol=1e-6)
        np.testing.assert_allclose(got.x, ref["x"], rtol=1e-5, atol=1e-8 * np.abs(ref["x"]).max())
    finally:
        prob.close()


# ---- bench.py --gpus N starts its own ranks --------------------------------------------------------------------
def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: two ranks (here both on the one GPU of
    the test box, gloo backend -- RCCL refuses two ranks on one device) and n_gpus: 2 in the line."""
    env = dict(os.environ, PREALPS_BENCH_BACKEND="gloo", PREALPS_BENCH_ONE_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "poisson",
                        "--n", "32", "--box", "4,4,8", "--steps", "10", "--warmup", "2", "--full", "--no-cpu",
                        "--spmm-reps", "3", "--phase-iters", "4"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["config"]["comm"] == "torch.gloo"
    assert len(out["config"]["halo_rows_per_rank"]) == 2 and min(out["config"]["halo_rows_per_rank"]) > 0
    assert out["value"] > 0 and "operator" in out["phases"]["device_us_per_iteration"]
    # a launcher that started the wrong number of ranks is refused
    env1 = dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True,
                       text=True, env=env1, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_bench_plain_run_dumps_the_timed_path_outputs(tmp_path):
    """A plain `bench.py` run reports the headline figures only (the passes of --full stay off), times exactly
    --steps steps, and --dump-outputs writes the solver's state after its last step: 2 warm-up + 10 timed steps
    of a solve that needs more, so X, R and x = X 1 are those of the oracle's 12th iteration."""
    from oracle import oracle as O
    from prealps_amd import gen
    n, box, t, its = 32, (4, 4, 8), 4, 12
    d = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "poisson",
                        "--n", str(n), "--box", "4,4,8", "--t", str(t), "--steps", "10", "--warmup", "2",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 10 and out["ms_per_step"] > 0
    np.testing.assert_allclose(out["value"] * out["ms_per_step"], 1e3, rtol=1e-9)
    assert not {"phases", "roofline", "block_jacobi", "parity", "cpu_baseline", "survey_nparts"} & set(out)
    assert out["config"]["restarts_in_timed_region"] == 0
    got = {f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d))}
    assert set(got) == {"x", "X", "R", "res"} and all(v.dtype == np.float64 for v in got.values())
    rp, ci, v = gen.poisson3d_csr(n)
    part, nparts = gen.box_partition(n, box)
    A = sp.csr_matrix((v, ci, rp), shape=(n ** 3, n ** 3))
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, nparts)
    ref = O.ECG(B, rowpos, t, max_iter=its).solve(O.reference_rhs(rowpos))
    assert ref["iters"] == its
    assert got["X"].shape == (n ** 3, t) and got["R"].shape == (n ** 3, t)
    np.testing.assert_allclose(got["res"][0], ref["final_res"], rtol=1e-8)
    np.testing.assert_allclose(np.linalg.norm(got["R"]), got["res"][0], rtol=1e-8)
    np.testing.assert_allclose(got["X"].sum(axis=1), got["x"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got["x"], ref["x"], rtol=1e-7, atol=1e-10 * np.abs(ref["x"]).max())


# ---- opt-in kernel variants (their switches are read once per process: run in a child) ---------------
_VARIANT_SNIPPET = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import prealps_amd
from oracle import oracle as O
A = O.poisson3d(16)
part = O.contiguous_partition(16 ** 3, 16)
rp, ci, v = O.as_csr(A)
prob = prealps_amd.EcgProblem(rp, ci, v, 16, part, scale=True, device=0)
B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, 16)
for t in (4, 8, 16):
    X = np.random.default_rng(t).standard_normal((B.shape[0], t))
    ref = O.spmm(B, X)
    np.testing.assert_allclose(prob.block_operator(X, t), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    zr = O.BlockJacobi(B, rowpos).apply(X)
    np.testing.assert_allclose(prob.block_jacobi_apply(X, t), zr, rtol=1e-9, atol=1e-10 * np.abs(zr).max())
rhs = prob.reference_rhs()
got = prob.solve(rhs, 8)
ref = O.ECG(B, rowpos, 8).solve(rhs)
assert got.iters == ref["iters"]
# (8 directions on 16 slabs: the t x t blocks lose rank as the solve converges, and the last residuals
# amplify rounding differences -- 5e-9 with k_bj_mfma, 2e-8 with bj_g4 at the final iteration, 1e-11 before)
np.testing.assert_allclose(got.res[:-2], ref["res"][:-2], rtol=1e-8)
np.testing.assert_allclose(got.res, ref["res"], rtol=1e-6)
prob.close()
# narrow bands (register-set class 2): 27 boxes of 4 x 4 x 4 points
from prealps_amd import gen
A2 = O.poisson3d(12)
part2, P2 = gen.box_partition(12, (4, 4, 4))
rp, ci, v = O.as_csr(A2)
prob2 = prealps_amd.EcgProblem(rp, ci, v, P2, part2, scale=True, device=0)
B2, perm2, rowpos2 = O.permute_by_part(O.symrac_scale(A2), part2, P2)
for t in (2, 4, 8, 16):      # (8 and 16: the matrix-core kernels, or -- PREALPS_BJ_MFMA=0 -- the register recurrence)
    X = np.random.default_rng(t).standard_normal((B2.shape[0], t))
    zr = O.BlockJacobi(B2, rowpos2).apply(X)
    np.testing.assert_allclose(prob2.block_jacobi_apply(X, t), zr, rtol=1e-9, atol=1e-10 * np.abs(zr).max())
print("variant ok", prob.stat("spmm_staged"), prob.stat("bj_max_bandwidth"), prob2.stat("bj_max_bandwidth"))
"""


@pytest.mark.parametrize("env", [{"PREALPS_SPMM_STAGED": "0"},
                                 {"PREALPS_BJ_MFMA": "0", "PREALPS_BJ_WIDE_FROM": "448"},
                                 {"PREALPS_BJ_MFMA": "2", "PREALPS_BJ_WIDE_FROM": "448", "PREALPS_TRSM_MFMA": "0"},
                                 {"PREALPS_ECG_FUSE": "0"},
                                 {"PREALPS_BJ_PAIRS": "0"},
                                 {"PREALPS_ECG_POLL": "1", "PREALPS_SPMM_GRAM": "1"},
                                 {"PREALPS_ECG_LAZY_STOP": "0"},
                                 {"PREALPS_ECG_LAZY_NORM": "0"}])
def test_opt_in_kernel_variants(env):
    """The window SpMM kernel on a matrix that would get the staged plan, the register recurrence of the
    block solve at 8 and 16 columns (PREALPS_BJ_MFMA=0), the matrix-core block solve at every width, the four-pass
    first half, the narrow-band sweep on plain instead of paired records, and the host polling for the residual norm
    (the default of multi-process runs) in one process, and the stopping test right after the update
    (PREALPS_ECG_LAZY_STOP=0) instead of one half-step later, and P / AP normalised in place as the reference does
    (PREALPS_ECG_LAZY_NORM=0; the default leaves them raw and applies U^-1 downstream): same answers as the oracle
    (Poisson 16^3, 16 slabs, band 256 -> register-set class 5; Poisson 12^3 in 27 boxes, class 2)."""
    r = subprocess.run([sys.executable, "-c", _VARIANT_SNIPPET % ROOT], capture_output=True, text=True,
                       env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0 and "variant ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


# ---- one solver after the other in one process, wide panels ---------------------------------------------------
@pytest.mark.parametrize("t", [8, 16, 4])
def test_variants_in_turn_share_the_gram_buffers(t):
    """Orthodir, Orthomin, fused Orthodir and the reductions one after the other on the same problem object: the
    sums of the wide Gram blocks (k_finish_wide) keep their shares and their ticket in the Gram buffer, two-panel
    products ([AP | R]^T P, [AP | AP_prev]^T Z) and one-panel products (Orthomin's AP^T Z) in turn.  (Round 4 had
    the ticket at an offset that depended on the block size: Orthomin behind Orthodir found share data where it
    looked for its ticket and stopped after one iteration with a zero residual -- on a problem no test ran.)"""
    import prealps_amd as pa
    from oracle import oracle as O
    A, part, nparts = _elasticity(12, (2, 3, 4))
    prob, B, rowpos = _problem(A, nparts, part)
    try:
        rhs = prob.reference_rhs()
        for name, red in (("odir", False), ("omin", False), ("odir", False), ("fused", False), ("omin", True), ("odir", True), ("omin", False)):
            a = _algs(name)
            try:
                ref = O.ECG(B, rowpos, t, a[1], O.ADAPT_BS if red else O.NO_BS_RED, 1e-5, 40).solve(rhs)
            except RuntimeError:
                # (16 directions on this small problem: P^T A P loses rank and Orthomin gives up, in the reference
                # -- src/solvers/ecg.c:318-322 -- in the oracle and here alike)
                with pytest.raises(pa.PreAlpsError):
                    prob.solve(rhs, t, ortho_alg=a[0], bs_red=pa.ADAPT_BS if red else pa.NO_BS_RED, max_iter=40)
                continue
            got = prob.solve(rhs, t, ortho_alg=a[0], bs_red=pa.ADAPT_BS if red else pa.NO_BS_RED, max_iter=40)
            assert got.iters == ref["iters"], (name, red, got.iters, ref["iters"])
            np.testing.assert_allclose(got.res[:12], ref["res"][:12], rtol=RTOL_HIST, err_msg="%s red=%s" % (name, red))
    finally:
        prob.close()


@pytest.mark.parametrize("kind", ["elasticity_boxes", "poisson_boxes", "poisson_slabs"])
def test_every_width_and_variant_in_turn_on_one_object(kind):
    """The same problem object through every panel width 1 .. 16 and every variant (Orthodir, Orthomin, fused
    Orthodir, with and without block-size reduction), one solve after the other: first residuals and iteration
    counts against the oracle (where the oracle breaks down -- Orthomin with P^T A P singular up to rounding --
    nothing is compared).  Complements the per-variant tests, each of which starts from a fresh object."""
    import prealps_amd as pa
    from oracle import oracle as O
    if kind == "elasticity_boxes":
        A, part, nparts = _elasticity(10, (2, 2, 5))
    elif kind == "poisson_boxes":
        from prealps_amd import gen
        rp, ci, v = gen.poisson3d_csr(20)
        part, nparts = gen.box_partition(20, (5, 5, 10))
        A = sp.csr_matrix((v, ci, rp), shape=(8000, 8000))
    else:
        A, part, nparts = O.poisson3d(16), None, 16
    prob, B, rowpos = _problem(A, nparts, part)
    try:
        rhs = prob.reference_rhs()
        checked = 0
        for t in (4, 8, 1, 16, 3, 2, 12, 5):
            for name in ("odir", "omin", "fused"):
                for red in (False, True):
                    if name == "fused" and red and t > 4:
                        continue                      # (fused + reduction at wide panels: covered where it is pinned)
                    a = _algs(name)
                    kw = dict(ortho_alg=a[0], bs_red=pa.ADAPT_BS if red else pa.NO_BS_RED, max_iter=25)
                    try:
                        ref = O.ECG(B, rowpos, t, a[1], O.ADAPT_BS if red else O.NO_BS_RED, 1e-5, 25).solve(rhs)
                    except RuntimeError:
                        # a breakdown (16 directions on 16 slabs: P^T A P is singular up to rounding, and whether its
                        # factorisation fails is decided in the last bit): either outcome here, nothing is compared
                        try:
                            prob.solve(rhs, t, **kw)
                        except pa.PreAlpsError:
                            pass
                        continue
                    got = prob.solve(rhs, t, **kw)
                    k = min(8, len(ref["res"]))
                    assert got.iters == ref["iters"], (kind, t, name, red, got.iters, ref["iters"])
                    np.testing.assert_allclose(got.res[:k], ref["res"][:k], rtol=1e-7, err_msg="%s t=%d %s red=%s" % (kind, t, name, red))
                    checked += 1
        assert checked >= 30
    finally:
        prob.close()


# ---- opt-in: HIP-graph replay of the iteration halves; the one-shard rehearsal ----------------------------
_GRAPH_SNIPPET = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import prealps_amd as pa
from prealps_amd import gen
from oracle import oracle as O
import scipy.sparse as sp
rp, ci, v = gen.elasticity3d_csr(9)
part, P = gen.box_partition_nodes(9, (3, 3, 3))
A = sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))
B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
prob.L.preAlps_hip_graphs(1)
rhs = prob.reference_rhs()
for alg_g, alg_o, t in ((pa.ORTHODIR, O.ORTHODIR, 4), (pa.ORTHOMIN, O.ORTHOMIN, 4), (pa.ORTHODIR, O.ORTHODIR, 8)):
    got = prob.solve(rhs, t, ortho_alg=alg_g, max_iter=400)
    ref = O.ECG(B, rowpos, t, alg_o, O.NO_BS_RED, 1e-5, 400).solve(rhs)
    assert got.iters == ref["iters"] and got.iters > 14, (got.iters, ref["iters"])      # (> 12 iterations: every phase replayed)
    np.testing.assert_allclose(got.res[:20], ref["res"][:20], rtol=1e-8)
    np.testing.assert_allclose(got.x, ref["x"], rtol=1e-5, atol=1e-7 * np.abs(ref["x"]).max())
prob.close()
print("graphs ok")
"""

_SHARD_SNIPPET = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import prealps_amd as pa
from prealps_amd import gen
from oracle import oracle as O
import scipy.sparse as sp
n, box, G, r, t = 12, (3, 3, 3), 4, 1, 4
rp, ci, v = gen.poisson3d_csr(n)
part, P = gen.box_partition(n, box)
A = sp.csr_matrix((v, ci, rp), shape=(n ** 3, n ** 3))
B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
p0, p1 = r * P // G, (r + 1) * P // G
lo, hi = int(rowpos[p0]), int(rowpos[p1])
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0, shard=(r, G))
assert prob.m == hi - lo and prob.stat("halo_rows") > 0
rhs = prob.reference_rhs()
got = prob.solve(rhs, t, max_iter=400)
# what the rehearsal iterates on: the rank's own diagonal block (halo rows arrive as zeros, sums are local),
# split into the rank's own subdomains
Brr = sp.csr_matrix(B[lo:hi][:, lo:hi])
ref = O.ECG(Brr, (rowpos[p0:p1 + 1] - lo).astype(np.int32), t, O.ORTHODIR, O.NO_BS_RED, 1e-5, 400).solve(rhs)
# (the enlarging columns of the rank's subdomains are p mod t in both: same splitting when p0 is a multiple of t)
assert p0 %% t == 0
assert got.iters == ref["iters"], (got.iters, ref["iters"])
np.testing.assert_allclose(got.res, ref["res"], rtol=1e-7)
np.testing.assert_allclose(got.x, ref["x"], rtol=1e-6, atol=1e-9 * np.abs(ref["x"]).max())
prob.close()
print("shard ok")
"""


_SPMM_GRAM_SNIPPET = r"""
import os, sys, numpy as np
sys.path.insert(0, %r)
import prealps_amd as pa
from prealps_amd import gen
from oracle import oracle as O
import scipy.sparse as sp
rp, ci, v = gen.elasticity3d_csr(9)
part, P = gen.box_partition_nodes(9, (3, 3, 3))
A = sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))
B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
rhs = None
for shard in (None, (0, 3)):
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0, **({"shard": shard} if shard else {}))
    rhs = prob.reference_rhs()
    if shard:      # the rank's own diagonal block (test_one_shard_rehearsal_solves_its_diagonal_block)
        p0, p1 = shard[0] * P // shard[1], (shard[0] + 1) * P // shard[1]
        lo, hi = int(rowpos[p0]), int(rowpos[p1])
        Bs, rps = sp.csr_matrix(B[lo:hi][:, lo:hi]), (rowpos[p0:p1 + 1] - lo).astype(np.int32)
        assert p0 %% 4 == 0
    else:
        Bs, rps = B, rowpos
    before, before_bj = prob.stat("spmm_gram_launches"), prob.stat("bj_gram_applies")
    for alg_g, alg_o in ((pa.ORTHODIR, O.ORTHODIR), (pa.ORTHOMIN, O.ORTHOMIN)):
        got = prob.solve(rhs, 4, ortho_alg=alg_g, max_iter=400)
        ref = O.ECG(Bs, rps, 4, alg_o, O.NO_BS_RED, 1e-5, 400).solve(rhs)
        assert got.iters == ref["iters"] and got.iters >= 8, (got.iters, ref["iters"])
        np.testing.assert_allclose(got.res[:20], ref["res"][:20], rtol=1e-8)
        np.testing.assert_allclose(got.x, ref["x"], rtol=1e-5, atol=1e-7 * np.abs(ref["x"]).max())
    on = os.environ["PREALPS_SPMM_GRAM"] == "1"
    assert prob.stat("spmm_runs") == 1.0
    if not shard:
        # a caller that drives the RCI protocol itself gets no Gram blocks from the SpMM / block solve (it may
        # change AP or Z between the library's routine and preAlps_ECGIterate) -- and the same residuals
        import ctypes as C
        import prealps_amd.lib as pl
        from prealps_amd.lib import check
        L = prob.L
        g0, b0 = prob.stat("spmm_gram_launches"), prob.stat("bj_gram_applies")
        e = prob.new_ecg(4, pl.ORTHODIR, pl.NO_BS_RED, 1e-5, 400)
        rci, stop = C.c_int(0), C.c_int(0)
        check(L.preAlps_ECGInitialize(C.byref(e), rhs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rci)), "init")
        check(L.preAlps_BlockJacobiApply(e.R, e.P), "bj")
        hist = []
        while stop.value != 1:
            if rci.value == 0:
                check(L.preAlps_BlockOperator(e.P, e.AP), "op")
            else:
                check(L.preAlps_ECGStoppingCriterion(C.byref(e), C.byref(stop)), "stop")
                hist.append(e.res)
                if stop.value == 1: break
                check(L.preAlps_BlockJacobiApply(e.AP, e.Z), "bj")
            check(L.preAlps_ECGIterate(C.byref(e), C.byref(rci)), "iterate")
        sol = (C.c_double * prob.m)()
        check(L.preAlps_ECGFinalize(C.byref(e), sol), "fin")
        ref = O.ECG(Bs, rps, 4, O.ORTHODIR, O.NO_BS_RED, 1e-5, 400).solve(rhs)
        assert len(hist) == ref["iters"], (len(hist), ref["iters"])
        np.testing.assert_allclose(hist[:20], ref["res"][:20], rtol=1e-8)
        if os.environ.get("PREALPS_RCI_FUSE") == "1" and on:
            # the caller has promised to call nothing but the library's two routines between the solver's steps
            # (INTEGRATION.md section 1): the same blocks as in the library's own loops, the same residuals
            assert prob.stat("spmm_gram_launches") - g0 >= len(hist) - 1 and prob.stat("bj_gram_applies") - b0 >= len(hist) - 2
        else:
            assert prob.stat("spmm_gram_launches") == g0 and prob.stat("bj_gram_applies") == b0
    assert (prob.stat("spmm_gram_launches") - before >= 16) if on else (prob.stat("spmm_gram_launches") == before)
    # the block solve leaves beta = [AP | AP_prev]^T Z behind in the Orthodir solve (every block in one bj_g4 class)
    assert (prob.stat("bj_gram_applies") - before_bj >= 8) if on else (prob.stat("bj_gram_applies") == before_bj)
    prob.close()
print("spmm gram ok")
"""


@pytest.mark.parametrize("on", ["1", "0", "1+rci"])
def test_spmm_and_block_solve_leave_the_gram_blocks_behind(on):
    """The defaults at 4 columns: k_spmm_runs_gram forms [AP | R]^T P while it computes AP (one partial block per
    workgroup) and k_bj_g4 forms [AP | AP_prev]^T Z while Z is in its registers (one per subdomain), k_finish32
    sums them: Orthodir and Orthomin, in one process and in the one-shard rehearsal, where the interior and the
    halo-reading halves of the SpMM each leave their share.  "0": both switched off (PREALPS_SPMM_GRAM,
    PREALPS_BJ_GRAM), the separate Gram kernels give the same answers."""
    env = dict(os.environ, PREALPS_SPMM_GRAM=on[0], PREALPS_BJ_GRAM=on[0])
    if on == "1+rci":        # PREALPS_RCI_FUSE=1: the same hand-over for a caller that drives the RCI loop itself
        env["PREALPS_RCI_FUSE"] = "1"
    r = subprocess.run([sys.executable, "-c", _SPMM_GRAM_SNIPPET % ROOT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "spmm gram ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])


def test_hip_graph_replay_matches_the_oracle():
    """PREALPS_ECG_GRAPH / preAlps_hip_graphs(1): the two halves of an iteration captured on their second pass
    and replayed afterwards (six pointer-rotation phases), Orthodir and Orthomin, 4 and 8 columns."""
    r = subprocess.run([sys.executable, "-c", _GRAPH_SNIPPET % ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "graphs ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_one_shard_rehearsal_solves_its_diagonal_block(overlap):
    """preAlps_hip_loopback (bench.py --shard-of): rank 1 of 4 in one process runs the real multi-process
    choreography (pack, exchange on the main stream and one SpMM launch -- or, PREALPS_HALO_OVERLAP=1,
    side-stream exchange beside the interior blocks, then the halo-reading ones) with zero halo rows and
    local sums: it must solve exactly the system of its own diagonal block."""
    r = subprocess.run([sys.executable, "-c", _SHARD_SNIPPET % ROOT], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PREALPS_HALO_OVERLAP=overlap))
    assert r.returncode == 0 and "shard ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
