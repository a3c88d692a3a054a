"""Single-precision storage of the one-copy band records (bj_g4.hip): PREALPS_BJ_BAND_PRECISION=single,
preAlps_hip_set_band_precision(32), EcgProblem.create_block_jacobi(band_precision="single").  The strictly lower part
of Lt = L D^-1 is rounded to fp32 once, D^-2 stays fp64, every entry is widened before the matrix cores see it and both
sweeps read the same record: half the bytes for the launches on panels of up to 4 (8) columns, a block solve that is
still symmetric positive definite.  Independent of PREALPS_BJ_ND_PRECISION; unset, everything computes the same bits as
before.

PREALPS_BJ_G4_RING and PREALPS_BJ_G4_WIDE are read once per process by the library, so every case that sets one of
them runs in a child process that gets them in its environment (one child per ring depth, looping over its cases and
ending at its first failed assert); the child prints, for every launch it checks, the ring depth, the storage bits and
whether the pipelined few-blocks chain ran (stats bj_g4_last_*), and the parent checks that the intended kernel was
reached.  A child killed by a signal or by its time limit fails the test, and no further child is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SW = "PREALPS_BJ_BAND_PRECISION"
RTOL_HIST = 1e-8            # (test_gpu_configs.py / test_gpu_parity.py)

FOUR = [(20, (5, 5, 10), 4), (24, (4, 4, 12), 4), (12, (6, 6, 6), 4), (24, (6, 4, 8), 3), (24, (8, 3, 8), 2),
        (24, (8, 8, 3), 1), (21, (7, 7, 3), 4), (20, (5, 5, 2), 4), (18, (9, 9, 3), 4), (20, (10, 10, 2), 4)]
EIGHT = [(20, (5, 5, 10), 8), (24, (4, 4, 12), 8), (12, (6, 6, 6), 7), (24, (8, 3, 8), 5), (24, (6, 4, 8), 6),
         (16, (4, 4, 8), 8)]


def _problem(A, P, part):
    import prealps_amd
    from oracle import oracle as O
    part = O.contiguous_partition(A.shape[0], P) if part is None else part
    rp, ci, v = O.as_csr(A)
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
    return prob, B, rowpos


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _poisson_boxes(n, box):
    from prealps_amd import gen
    rp, ci, v = gen.poisson3d_csr(n)
    part, P = gen.box_partition(n, box)
    return sp.csr_matrix((v, ci, rp), shape=(n ** 3, n ** 3)), P, part


def _elasticity_boxes(nn, box=(4, 4, 4)):
    from prealps_amd import gen
    rp, ci, v = gen.elasticity3d_csr(nn)
    part, P = gen.box_partition_nodes(nn, box)
    N = len(rp) - 1
    return sp.csr_matrix((v, ci, rp), shape=(N, N)), P, part


def _mixed(monkeypatch):
    """One sparse block (5600 rows) beside band blocks of 200 rows (test_gpu_nd_precision.py's "mixed")."""
    from oracle import oracle as O
    n = 20
    idx = np.arange(n ** 3)
    part = np.where(idx // (n * n) < 14, 0, 1 + (idx - 14 * n * n) // 200).astype(np.int32)
    monkeypatch.setenv("PREALPS_ND_LEAF", "40")
    monkeypatch.setenv("PREALPS_BJ_ND", "2")
    return O.poisson3d(n), int(part.max()) + 1, part


# ---- the children -------------------------------------------------------------------------------------------
_CHILD_HEAD = r"""
import json, os, sys
import numpy as np, scipy.sparse as sp
sys.path.insert(0, %r)
import prealps_amd as pa
from prealps_amd import gen
from oracle import oracle as O

def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))

def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))

def build(kind, n, box):
    if kind == "poisson":
        rp, ci, v = gen.poisson3d_csr(n)
        part, P = gen.box_partition(n, tuple(box))
        N = n ** 3
    else:
        rp, ci, v = gen.elasticity3d_csr(n)
        part, P = gen.box_partition_nodes(n, tuple(box))
        N = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
    return prob, B, rowpos

def launch(prob):
    return dict(ring=int(prob.stat("bj_g4_last_ring")), bits=int(prob.stat("bj_g4_last_bits")),
                pipelined=int(prob.stat("bj_g4_last_pipelined")))
"""

_APPLY_CHILD = _CHILD_HEAD + r"""
for kind, n, box, t in json.loads(os.environ["BAND_CASES"]):
    prob, B, rowpos = build(kind, n, box)
    X = np.random.default_rng(n + t).standard_normal((prob.m, t))
    prob.create_block_jacobi(band_precision="double")
    assert prob.stat("bj_band_precision") == 64
    zd = prob.block_jacobi_apply(X, t)
    ld, g4_d, fac_d = launch(prob), prob.stat("bj_g4_bytes"), prob.stat("bj_factor_bytes")
    prob.create_block_jacobi(band_precision="single")
    assert prob.stat("bj_band_precision") == 32
    zs = prob.block_jacobi_apply(X, t)
    ls, g4_s, fac_s = launch(prob), prob.stat("bj_g4_bytes"), prob.stat("bj_factor_bytes")
    again = all(same_bits(zs, prob.block_jacobi_apply(X, t)) for _ in range(3))
    wmax = int(prob.stat("bj_max_bandwidth"))
    prob.close()
    zo = O.BlockJacobi(B, rowpos).apply(X)
    d, do = rel(zs, zd), rel(zs, zo)
    print("CASE " + json.dumps(dict(kind=kind, n=n, box=box, t=t, d=d, d_oracle=do, wmax=wmax, double=ld, single=ls)), flush=True)
    assert g4_d > 0 and g4_s == g4_d / 2 and fac_s == fac_d, (g4_d, g4_s, fac_d, fac_s)
    assert np.isfinite(zs).all()
    assert 1e-10 < d < 1e-6, d
    assert 1e-10 < do < 1e-6, do
    assert again, "repeated applies differ"
    assert ld["bits"] == 64 and ls["bits"] == 32 and ls["pipelined"] == 0, (ld, ls)
print("band apply ok")
"""

_GRAM_CHILD = _CHILD_HEAD + r"""
for kind, n, box in json.loads(os.environ["BAND_CASES"]):
    prob, B, rowpos = build(kind, n, box)
    prob.create_block_jacobi(band_precision="single")
    assert prob.stat("bj_band_precision") == 32
    rhs = prob.reference_rhs()
    before = prob.stat("bj_gram_applies")
    got = prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, tol=1e-5, max_iter=1000)
    print("CASE " + json.dumps(dict(kind=kind, n=n, box=box, iters=int(got.iters), res=[float(r) for r in got.res],
                                    gram_applies=int(prob.stat("bj_gram_applies") - before), single=launch(prob))), flush=True)
    prob.close()
print("band gram ok")
"""


def _run_child(snippet, env, timeout):
    """One child under its own time limit; a child that was killed (signal or time limit) fails the test at once."""
    try:
        r = subprocess.run([sys.executable, "-c", snippet % ROOT], capture_output=True, text=True, timeout=timeout,
                           env=dict(os.environ, **env))
    except subprocess.TimeoutExpired as e:
        pytest.fail("child exceeded its time limit of %d s: %s" % (timeout, str(e.stderr or "")[-1500:]), pytrace=False)
    if r.returncode < 0:
        pytest.fail("child killed by signal %d: %s" % (-r.returncode, r.stderr[-2500:]), pytrace=False)
    cases = [json.loads(l[5:]) for l in r.stdout.splitlines() if l.startswith("CASE ")]
    return r, cases


def _ring_allowed(req, wmax):
    """The launch planner's (bj_g4_plan.c) cap on the ring depth for fp32 records of band wmax: at most 15 LDS-DMA pieces of 1 KiB in flight
    and at most 40 KiB of LDS per wavefront."""
    nld = (32 * (wmax + 4) + 1023) // 1024
    ring = req
    while ring > 2 and ((ring - 1) * nld > 15 or ring * nld * 1024 > 40 * 1024):
        ring //= 2
    return ring


# ---- 1. the apply in every dispatch class -----------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["2", "default", "4", "8"])
def test_single_precision_apply_in_every_dispatch_class(ring):
    """Panels of 1 .. 4 columns (one column set) and 5 .. 8 columns (two sets, PREALPS_BJ_G4_WIDE=1) on 12 / 14 / 16
    register tiles, Poisson boxes and elasticity 12^3 in blocks of 192 rows (the headline's block shape), with the
    memory-bound kernel (PREALPS_BJ_G4_RING=2), the few-blocks path (default: fp32 records take the plain chain with the
    deep ring) and, for the 4-column cases, rings of 4 and 8 buffers.  fp64 then fp32 records on the same problem:
    bj_band_precision 64 / 32, bj_g4_bytes exactly halved, bj_factor_bytes unchanged, and the fp32 apply differs from
    the fp64 one and from the oracle's exact block solve by fp32 rounding of the coefficients: 1e-10 < d < 1e-6.
    Three more applies give the same bits.  Measured (MI355X): Poisson 0.95-1.16e-8, elasticity 12^3 5.3-6.1e-8
    (band 65; against the oracle: the same figures to four digits), the same at every ring depth."""
    cases = [("poisson", n, list(box), t) for n, box, t in FOUR] + [("elasticity", 12, [4, 4, 4], t) for t in (1, 2, 4)]
    if ring in ("2", "default"):
        cases += [("poisson", n, list(box), t) for n, box, t in EIGHT] + [("elasticity", 12, [4, 4, 4], 8)]
    env = {"PREALPS_BJ_WIDE_FROM": "448", "PREALPS_BJ_G4_WIDE": "1", "BAND_CASES": json.dumps(cases)}
    if ring != "default":
        env["PREALPS_BJ_G4_RING"] = ring
    r, seen = _run_child(_APPLY_CHILD, env, 900)
    for c in seen:
        print("ring %s  %s %d %s t=%d: single / double %.3e, single / oracle %.3e, band %d, launches %s %s"
              % (ring, c["kind"], c["n"], c["box"], c["t"], c["d"], c["d_oracle"], c["wmax"], c["double"], c["single"]))
    assert r.returncode == 0 and "band apply ok" in r.stdout, (r.stdout[-1500:], r.stderr[-2500:])
    assert len(seen) == len(cases)
    req = 8 if ring == "default" else int(ring)
    for c in seen:
        # the widest class runs last or not, so the cap of the widest band bounds the depth from below
        lo = _ring_allowed(req, c["wmax"])
        assert lo <= c["single"]["ring"] <= req, (c, req)
        if ring == "2":
            assert c["single"]["ring"] == 2 and c["double"]["ring"] == 2 and c["double"]["pipelined"] == 0, c


# ---- 2. symmetric positive definite ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_single_precision_band_solve_is_symmetric_positive_definite(kind, monkeypatch):
    """Both sweeps read the same rounded record and D^-2 sits between them in fp64: Lt32^-T D^-2 Lt32^-1 is symmetric
    positive definite to fp64 roundoff: y^T M x = x^T M y, x^T M x > 0."""
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    A, P, part = _poisson_boxes(24, (4, 4, 12)) if kind == "poisson" else _elasticity_boxes(12)
    prob, B, rowpos = _problem(A, P, part)
    rng = np.random.default_rng(11)
    try:
        prob.create_block_jacobi(band_precision="single")
        assert prob.stat("bj_band_precision") == 32
        for _ in range(3):
            X = rng.standard_normal((prob.m, 2))
            Z = prob.block_jacobi_apply(X, 2)
            assert prob.stat("bj_g4_last_bits") == 32
            x, y, mx, my = X[:, 0], X[:, 1], Z[:, 0], Z[:, 1]
            assert abs(y @ mx - x @ my) <= 1e-10 * np.linalg.norm(y) * np.linalg.norm(mx)
            assert x @ mx > 0 and y @ my > 0
    finally:
        prob.close()


# ---- 3. the Gram by-product -------------------------------------------------------------------------------------
def test_gram_by_product_of_the_single_precision_launch():
    """Orthodir t = 4 in the library's loop with fp32 records: the launch that leaves [AP | AP_prev]^T Z behind
    (PREALPS_BJ_GRAM=1) and the plain one followed by the separate Gram kernels (=0), at the default ring and rings of
    2 / 4 / 8 buffers, every combination in a child of its own: equal iteration counts, and residual histories to 1e-8
    over their first 20 entries -- the comparison of test_spmm_and_block_solve_leave_the_gram_blocks_behind, whose
    RTOL_HIST this is.  The two ways of forming the Gram block differ in summation order only (1e-16 relative in beta);
    the recurrence carries that difference at a constant absolute size while the residual falls by 4e5, so the LAST
    entries of a history agree to fewer digits than the first: measured (MI355X, default ring, elasticity 12^3, 39
    entries) the last two differ by 2.3e-8 relative (1.5e-12 absolute, of a first entry of 24.0), the other 37 by less
    than 1e-8; Poisson 24^3 / 20^3 (25 / 21 entries) agree to 1e-8 throughout.  The whole history is therefore held
    to 1e-6: a stale row of AP_prev in the launch (the load that the chunk waits do not cover at ring >= 4) puts an
    error of the order of 1e-3 into beta (one tile of one block of a sum over 27 blocks x 12 tiles) and would move
    the history in its third to sixth digit and, as a rule, the iteration count.
    Blocks of 256 / 250 / 192 rows: the 16-tile unit (Poisson 20^3 in boxes of 5 x 5 x 10), 12 tiles."""
    cases = [("poisson", 24, [4, 4, 12]), ("poisson", 20, [5, 5, 10]), ("elasticity", 12, [4, 4, 4])]
    ref, on_applies = None, 0
    for ring in ("default", "2", "4", "8"):
        for gram in ("0", "1"):
            env = {"PREALPS_BJ_WIDE_FROM": "448", "PREALPS_BJ_GRAM": gram, "BAND_CASES": json.dumps(cases)}
            if ring != "default":
                env["PREALPS_BJ_G4_RING"] = ring
            r, seen = _run_child(_GRAM_CHILD, env, 600)
            assert r.returncode == 0 and "band gram ok" in r.stdout, (ring, gram, r.stdout[-500:], r.stderr[-2500:])
            assert len(seen) == len(cases)
            for c in seen:
                print("ring %s gram %s  %s %d: %d iterations, %d applies left the Gram block, launch %s"
                      % (ring, gram, c["kind"], c["n"], c["iters"], c["gram_applies"], c["single"]))
                assert c["single"]["bits"] == 32 and c["single"]["pipelined"] == 0, c
                if ring != "default":
                    assert c["single"]["ring"] <= int(ring)
                if gram == "0":
                    assert c["gram_applies"] == 0, c
                else:
                    on_applies += c["gram_applies"]
            if ref is None:
                ref = seen
            for c, c0 in zip(seen, ref):
                assert c["iters"] == c0["iters"], (ring, gram, c["kind"], c["n"], c["iters"], c0["iters"])
                d = np.abs(np.array(c["res"]) - np.array(c0["res"])) / np.array(c0["res"])
                print("ring %s gram %s  %s %d: history against the first child's: first 20 entries %.2e, all %.2e (entry %d of %d)"
                      % (ring, gram, c["kind"], c["n"], d[:20].max(), d.max(), int(d.argmax()), len(d)))
                np.testing.assert_allclose(c["res"][:20], c0["res"][:20], rtol=RTOL_HIST)
                np.testing.assert_allclose(c["res"], c0["res"], rtol=1e-6)
    assert on_applies > 0            # the by-product launch did run


# ---- 4. ECG ------------------------------------------------------------------------------------------------------
def _ecg(kind, monkeypatch):
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    if kind == "poisson":
        return _poisson_boxes(24, (4, 4, 12))
    if kind == "elasticity12":
        return _elasticity_boxes(12)
    if kind == "elasticity16":
        return _elasticity_boxes(16)
    if kind == "elasticity24":
        return _elasticity_boxes(24)
    return _mixed(monkeypatch)


@pytest.mark.parametrize("t", [4, 8])
@pytest.mark.parametrize("alg", ["odir", "omin"])
@pytest.mark.parametrize("kind", ["poisson", "elasticity12", "elasticity24", "mixed", "elasticity16"])
def test_ecg_with_single_precision_band_records(kind, alg, t, monkeypatch):
    """ECG with the fp32 records converges to tol; the true residual of x on the permuted, scaled matrix is within
    2 sqrt(t) tol, and the iteration count within max(2, 3 %) of the oracle's fp64 count.  "mixed": one sparse block
    beside band blocks, both switches single.  Elasticity 16^3 is run and printed but its count is not compared: plain
    PCG on it moves by 2.6 % under perturbations of this size (convergence and the residual bound are asserted)."""
    import prealps_amd as pa
    from oracle import oracle as O
    ga, oa = {"odir": (pa.ORTHODIR, O.ORTHODIR), "omin": (pa.ORTHOMIN, O.ORTHOMIN)}[alg]
    A, P, part = _ecg(kind, monkeypatch)
    prob, B, rowpos = _problem(A, P, part)
    tol = 1e-5
    try:
        prob.create_block_jacobi(band_precision="single", nd_precision="single" if kind == "mixed" else None)
        assert prob.stat("bj_band_precision") == 32
        if kind == "mixed":
            assert prob.stat("bj_nd_precision") == 32 and prob.stat("bj_nd_blocks") == 1
        rhs = prob.reference_rhs()
        got = prob.solve(rhs, t, ortho_alg=ga, tol=tol)
        assert prob.stat("bj_g4_last_bits") == 32
    finally:
        prob.close()
    ref = O.ECG(B, rowpos, t, ortho_alg=oa, tol=tol).solve(rhs)
    true_res = float(np.linalg.norm(rhs - B @ got.x) / np.linalg.norm(rhs))
    print("%s %s t=%d: %d iterations (fp64 oracle %d), true residual %.3e" % (kind, alg, t, got.iters, ref["iters"], true_res))
    assert got.iters < 1000
    assert true_res <= 2.0 * np.sqrt(t) * tol
    if kind != "elasticity16":
        assert abs(got.iters - ref["iters"]) <= max(2, 0.03 * ref["iters"])


# ---- 5. the default keeps its bits ------------------------------------------------------------------------------
def test_default_is_fp64_bit_for_bit(monkeypatch):
    """Unset, the records are fp64 and the apply has the bits of PREALPS_BJ_BAND_PRECISION=double;
    preAlps_hip_set_band_precision(64) overrides PREALPS_BJ_BAND_PRECISION=single, and 0 follows it again."""
    from prealps_amd.lib import check
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    prob, B, rowpos = _problem(*_poisson_boxes(24, (4, 4, 12)))
    X = np.random.default_rng(3).standard_normal((prob.m, 4))
    L = prob.L
    try:
        monkeypatch.delenv(SW, raising=False)
        prob.create_block_jacobi()
        assert prob.stat("bj_band_precision") == 64
        z_unset = prob.block_jacobi_apply(X, 4)
        monkeypatch.setenv(SW, "double")
        prob.create_block_jacobi()
        assert prob.stat("bj_band_precision") == 64
        assert _same_bits(prob.block_jacobi_apply(X, 4), z_unset)
        monkeypatch.setenv(SW, "single")
        check(L.preAlps_hip_set_band_precision(64), "preAlps_hip_set_band_precision")
        try:
            prob.create_block_jacobi()
            assert prob.stat("bj_band_precision") == 64
            assert _same_bits(prob.block_jacobi_apply(X, 4), z_unset)
        finally:
            L.preAlps_hip_set_band_precision(0)
        prob.create_block_jacobi()
        assert prob.stat("bj_band_precision") == 32
        assert not _same_bits(prob.block_jacobi_apply(X, 4), z_unset)
    finally:
        prob.close()


# ---- 6. independence of the two switches, and where the switch does not reach -----------------------------------
def test_sparse_switch_leaves_band_blocks_alone(monkeypatch):
    """PREALPS_BJ_ND_PRECISION=single on a band-only problem: bj_band_precision stays 64 and the bits are fp64's."""
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    prob, B, rowpos = _problem(*_poisson_boxes(24, (4, 4, 12)))
    X = np.random.default_rng(5).standard_normal((prob.m, 4))
    out = {}
    try:
        for v in ("double", "single"):
            monkeypatch.setenv("PREALPS_BJ_ND_PRECISION", v)
            prob.create_block_jacobi()
            assert prob.stat("bj_band_precision") == 64 and prob.stat("bj_nd_precision") == 0
            out[v] = prob.block_jacobi_apply(X, 4)
    finally:
        prob.close()
    assert _same_bits(out["single"], out["double"])


def test_band_switch_leaves_the_sparse_factor_alone(monkeypatch):
    """band_precision="single" alone on the mixed partition: the sparse block's factor stays fp64."""
    A, P, part = _mixed(monkeypatch)
    prob, B, rowpos = _problem(A, P, part)
    try:
        prob.create_block_jacobi(band_precision="single")
        assert prob.stat("bj_band_precision") == 32
        assert prob.stat("bj_nd_precision") == 64 and prob.stat("bj_nd_blocks") == 1
        prob.create_block_jacobi(nd_precision="single")
        assert prob.stat("bj_band_precision") == 64 and prob.stat("bj_nd_precision") == 32
    finally:
        prob.close()


def test_sixteen_columns_and_no_one_copy_records_keep_the_fp64_bits(monkeypatch):
    """t = 16 reads the plain fp64 records (k_bj_mfma): the fp64 bits with `single`.  PREALPS_BJ_G4=0: there are no
    one-copy records, the stat is 0 and the 4-column apply has the fp64 bits."""
    monkeypatch.setenv("PREALPS_BJ_WIDE_FROM", "448")
    prob, B, rowpos = _problem(*_poisson_boxes(16, (4, 4, 8)))
    X16 = np.random.default_rng(6).standard_normal((prob.m, 16))
    X4 = X16[:, :4].copy()
    try:
        prob.create_block_jacobi(band_precision="double")
        zd16, zd4 = prob.block_jacobi_apply(X16, 16), prob.block_jacobi_apply(X4, 4)
        prob.create_block_jacobi(band_precision="single")
        assert prob.stat("bj_band_precision") == 32
        assert _same_bits(prob.block_jacobi_apply(X16, 16), zd16)
        assert not _same_bits(prob.block_jacobi_apply(X4, 4), zd4)
        monkeypatch.setenv("PREALPS_BJ_G4", "0")
        prob.create_block_jacobi(band_precision="double")
        assert prob.stat("bj_band_precision") == 0 and prob.stat("bj_g4_bytes") == 0
        z0 = prob.block_jacobi_apply(X4, 4)
        prob.create_block_jacobi(band_precision="single")
        assert prob.stat("bj_band_precision") == 0 and prob.stat("bj_g4_bytes") == 0
        assert _same_bits(prob.block_jacobi_apply(X4, 4), z0)
    finally:
        prob.close()


# ---- 7. a bad value ----------------------------------------------------------------------------------------------
def test_bad_value_fails_create(monkeypatch):
    """PREALPS_BJ_BAND_PRECISION=half: create fails (return-code mode) and names the switch; a value given to the
    Python keyword does not read the switch at all."""
    import prealps_amd as pa
    monkeypatch.setenv(SW, "half")
    prob, B, rowpos = _problem(*_poisson_boxes(12, (6, 6, 6)))
    try:
        with pytest.raises(pa.PreAlpsError, match=SW):
            prob.create_block_jacobi()
        with pytest.raises(ValueError):
            prob.create_block_jacobi(band_precision="half")
        prob.create_block_jacobi(band_precision="single")
        assert prob.stat("bj_band_precision") == 32
    finally:
        prob.close()
