"""The PAIR launch of the band block solve (bj_g4.hip: two blocks of one class of identical blocks per wavefront, the
record read once for both; the tasks are bj_share.c's pa_bj_pair_tasks).  Per column it runs the same matrix
instructions on the same operands as the one-block launch, so everything here must come out in the same bytes.

Two fresh child processes run the same script, one with PREALPS_BJ_PAIR=1 (pair whenever a launch list has a pair)
and one with PREALPS_BJ_PAIR=0 (never), and leave every result in a file; the tests compare the two files.  Both run
with PREALPS_BJ_G4_RING=2, so that the unpaired launch is the plain chain of the many-blocks regime, the launch the
rule replaces: on the few blocks of these problems the default would be the pipelined few-blocks chain, which sums the
Gram rows of a block in ascending tile order where the plain chain -- and with it the PAIR launch -- sums them in
descending order (Z is the same bytes from all three; the Gram block, and so a solve's history, is not: measured on
the elasticity problem here, where the histories of the pipelined and the paired launch agree to 8 digits).

  * Poisson 12^3 in boxes of 5 x 5 x 10 (18 blocks, the 16-tile unit) and elasticity on (10, 16, 32) nodes in boxes of
    2 x 4 x 8 (80 blocks, the 12-tile unit), the problems of tests/test_gpu_bj_share.py: Z on panels of 1, 3 and 4
    columns, a solve of 10 iterations through the library's loop (the Gram partials of the apply feed its
    recurrence), bj_g4_last_paired and bj_paired_blocks against a numpy restatement.
  * Synthetic band blocks (gen.band_blocks_csr, the harness of tests/test_gpu_band_blocks.py), every block twice and
    one three times (an odd class: a half-empty task), rows 1, 7, 8, 9, 17, 191, 192, the widest band of the launch at
    1 and on both sides of every edge of the kernel's DQ parameter in the 12-tile unit (32 | 33, 48 | 49, 64 | 65,
    80 = the widest band the two-set kernels take): byte-equal to the unpaired result and inside the backward-error
    bound of that harness, omega_q <= (3 w_q + 16) u.
  * A refresh that splits one class (the apply must fall back to the one-block launch: a block that reads its own
    records again cannot be served from its partner's) and the refresh back (paired again)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
U = 2.0 ** -53
COLS = (1, 3, 4)
SOLVE_ITERS = 10
ROWS = (1, 7, 8, 9, 17, 191, 192)
BANDS = (1, 32, 33, 48, 49, 64, 65, 80)
KINDS = ("poisson12", "elasticity")


# ---- the problems ----------------------------------------------------------------------------------------------------
def _real(kind):
    import test_gpu_bj_share as S
    return S._matrix(kind)


@functools.lru_cache(maxsize=None)
def _synthetic(wmax):
    """(rp, ci, v, P, part, shapes): every shape (b, min(wmax, b - 1)) of ROWS twice, the copies a whole round apart so
    that no pair is made of neighbours, and (17, .) a third time."""
    from prealps_amd import gen
    shapes = [(b, min(wmax, b - 1)) for b in ROWS]
    rp, ci, v, part, P = gen.band_blocks_csr(shapes, 4000 + wmax)
    A = sp.csr_matrix((v, ci, rp))
    r0 = np.concatenate([[0], np.cumsum([b for b, _ in shapes])])
    diag = [A[r0[q]:r0[q + 1], r0[q]:r0[q + 1]] for q in range(P)]
    order = list(range(P)) + list(range(P)) + [ROWS.index(17)]
    M = sp.block_diag([diag[q] for q in order], format="csr")
    M.sort_indices()
    blocks = [shapes[q] for q in order]
    part = np.repeat(np.arange(len(order)), [b for b, _ in blocks]).astype(np.int32)
    return (M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64), len(order), part, blocks)


def _panels(m, seed):
    return {t: np.random.default_rng(seed + t).standard_normal((m, t)) for t in COLS}


# ---- the child: everything under the environment it was started with -------------------------------------------------
def _stats(prob):
    return {k: int(prob.stat(k)) for k in ("bj_pair_tasks", "bj_paired_blocks", "bj_g4_last_paired", "bj_shared_blocks",
                                            "bj_share_classes", "bj_parts_local", "bj_g4_bytes", "bj_max_bandwidth")}


def child_run(path):
    import prealps_amd
    arrays, info = {}, {}

    def problem(rp, ci, v, P, part):
        return prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)

    for kind in KINDS:
        rp, ci, v, P, part = _real(kind)
        prob = problem(rp, ci, v, P, part)
        try:
            prob.create_block_jacobi()
            X = _panels(prob.m, 300)
            for t in COLS:
                arrays["%s.Z%d" % (kind, t)] = prob.block_jacobi_apply(X[t], t)
                info["%s.paired%d" % (kind, t)] = int(prob.stat("bj_g4_last_paired"))
            info[kind + ".stats"] = _stats(prob)
            before = prob.stat("bj_gram_applies")
            got = prob.solve(prob.reference_rhs(), 4, ortho_alg=prealps_amd.ORTHODIR, tol=1e-30, max_iter=SOLVE_ITERS)
            arrays[kind + ".res"] = np.asarray(got.res, np.float64)
            arrays[kind + ".x"] = np.asarray(got.x, np.float64)
            info[kind + ".solve"] = dict(iters=int(got.iters), gram_applies=int(prob.stat("bj_gram_applies") - before),
                                         paired=int(prob.stat("bj_g4_last_paired")))
        finally:
            prob.close()

    for wmax in BANDS:
        rp, ci, v, P, part, blocks = _synthetic(wmax)
        prob = problem(rp, ci, v, P, part)
        try:
            prob.create_block_jacobi()
            X = _panels(prob.m, 500 + wmax)
            for t in COLS:
                arrays["band%d.Z%d" % (wmax, t)] = prob.block_jacobi_apply(X[t], t)
                info["band%d.paired%d" % (wmax, t)] = int(prob.stat("bj_g4_last_paired"))
            info["band%d.stats" % wmax] = _stats(prob)
        finally:
            prob.close()

    # the refresh sequence of tests/test_gpu_bj_share.py: doubled (classes survive), one in-block entry of a block that
    # reads another block's records halved (its class splits), doubled again
    rp, ci, v, P, part, v2, v3 = _refresh_values()
    prob = problem(rp, ci, v, P, part)
    try:
        prob.create_block_jacobi()
        X = _panels(prob.m, 700)
        for step, val in (("create", None), ("doubled", v2), ("split", v3), ("back", v2)):
            if val is not None:
                prob.update_values(val, precond="refactor")
            for t in COLS:
                arrays["refresh.%s.Z%d" % (step, t)] = prob.block_jacobi_apply(X[t], t)
            info["refresh." + step] = _stats(prob)
    finally:
        prob.close()

    np.savez(path + ".npz", **arrays)
    with open(path + ".json", "w") as f:
        json.dump(info, f)
    print("bj pair child ok")


def _refresh_values():
    import test_gpu_bj_share as S
    rp, ci, v, P, part = _real("poisson12")
    first = S._natural_classes(rp, ci, v, part, P)
    p = int(np.nonzero(first != np.arange(P))[0][0])          # a block that repeats an earlier one
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    e = int(np.nonzero((part[rows] == p) & (part[ci] == p) & (rows < ci))[0][0])
    i, j = int(rows[e]), int(ci[e])
    v2 = 2.0 * v
    v3 = v2.copy()
    v3[e] *= 0.5
    v3[np.nonzero((rows == j) & (ci == i))[0][0]] *= 0.5
    return rp, ci, v, P, part, v2, v3


_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import test_gpu_bj_pair as T
T.child_run(sys.argv[1])
"""


class _Run:
    def __init__(self, path):
        self.a = dict(np.load(path + ".npz"))
        with open(path + ".json") as f:
            self.i = json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(paired, unpaired): one child each; a child that was killed or timed out fails here and the other is not started"""
    tmp = tmp_path_factory.mktemp("bj_pair")
    out = []
    for mode in ("1", "0"):
        path = str(tmp / ("pair" + mode))
        env = dict(os.environ, PREALPS_BJ_PAIR=mode, PREALPS_BJ_ND="0", PREALPS_BJ_G4_RING="2")
        try:
            r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT), path], capture_output=True, text=True,
                               timeout=240, env=env)
        except subprocess.TimeoutExpired as e:
            pytest.fail("child PREALPS_BJ_PAIR=%s exceeded its time limit: %s" % (mode, str(e.stderr or "")[-1500:]), pytrace=False)
        if r.returncode < 0:
            pytest.fail("child PREALPS_BJ_PAIR=%s killed by signal %d: %s" % (mode, -r.returncode, r.stderr[-2500:]), pytrace=False)
        assert r.returncode == 0 and "bj pair child ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
        out.append(_Run(path))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _paired_ref(classes):
    """blocks with a partner when every class pairs its members two by two"""
    _, n = np.unique(np.asarray(classes), return_counts=True)
    return int(np.sum(2 * (n // 2)))


# ---- the two problems of tests/test_gpu_bj_share.py -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_identical_boxes_in_pairs_give_the_same_bytes(runs, kind):
    import test_gpu_bj_share as S
    on, off = runs
    rp, ci, v, P, part = _real(kind)
    first = S._natural_classes(rp, ci, v, part, P)
    s1, s0 = on.i[kind + ".stats"], off.i[kind + ".stats"]
    print("%s: %d blocks, %d share in %d classes; %d tasks, %d blocks with a partner (restatement %d)"
          % (kind, P, s1["bj_shared_blocks"], s1["bj_share_classes"], s1["bj_pair_tasks"], s1["bj_paired_blocks"], _paired_ref(first)))
    for t in COLS:
        assert on.i["%s.paired%d" % (kind, t)] == 1 and off.i["%s.paired%d" % (kind, t)] == 0, t
        Z1, Z0 = on.a["%s.Z%d" % (kind, t)], off.a["%s.Z%d" % (kind, t)]
        assert np.isfinite(Z1).all() and np.abs(Z1).max() > 0
        assert _same_bits(Z1, Z0), (kind, t)
    # The restatement pairs the natural-order classes.  The factor order may merge two of them (tests/test_gpu_bj_share.py:
    # Poisson 12^3 has 10 blocks that share in natural order, 11 in the library's), and merging classes never takes a
    # partner away: the library's count is the restatement's where it found the same number of sharing blocks, and at
    # least the restatement's and at most one pair more per merged class otherwise.  Every block is in exactly one task.
    merged = s1["bj_shared_blocks"] - int(np.count_nonzero(first != np.arange(P)))
    assert merged >= 0
    assert 0 < _paired_ref(first) <= s1["bj_paired_blocks"] <= _paired_ref(first) + 2 * merged
    assert s1["bj_paired_blocks"] % 2 == 0 and s1["bj_paired_blocks"] <= 2 * (P - s1["bj_share_classes"])
    assert s1["bj_pair_tasks"] == P - s1["bj_paired_blocks"] // 2
    assert s0["bj_paired_blocks"] == s1["bj_paired_blocks"] and s0["bj_pair_tasks"] == s1["bj_pair_tasks"]    # (built either way)


@pytest.mark.parametrize("kind", KINDS)
def test_a_short_solve_has_the_same_history(runs, kind):
    """Orthodir t = 4 through the library's loop: its apply is the launch that leaves the Gram block behind"""
    on, off = runs
    g1, g0 = on.i[kind + ".solve"], off.i[kind + ".solve"]
    print("%s: %d iterations, %d / %d applies left the Gram block, last launch paired %d / %d"
          % (kind, g1["iters"], g1["gram_applies"], g0["gram_applies"], g1["paired"], g0["paired"]))
    assert g1["iters"] == g0["iters"] and SOLVE_ITERS - 1 <= g1["iters"] <= SOLVE_ITERS + 1      # (stopped by max_iter)
    assert g1["gram_applies"] == g0["gram_applies"] > 0
    assert g1["paired"] == 1 and g0["paired"] == 0
    assert len(on.a[kind + ".res"]) >= SOLVE_ITERS - 1
    assert _same_bits(on.a[kind + ".res"], off.a[kind + ".res"])
    assert _same_bits(on.a[kind + ".x"], off.a[kind + ".x"])


# ---- synthetic band blocks ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _band_case(wmax):
    """what tests/test_gpu_band_blocks.py holds per case: the scaled B, and per block A_q and M = |L| |L|^T"""
    import test_gpu_band_blocks as T
    from oracle import oracle as O
    rp, ci, v, P, part, blocks = _synthetic(wmax)
    c = T._Case()
    c.blocks, c.P, c.N = blocks, P, len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(c.N, c.N))
    c.B, perm, c.rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
    assert np.array_equal(perm, np.arange(c.N))
    c.A, c.M = [], []
    for q in range(P):
        r0, r1 = c.rowpos[q], c.rowpos[q + 1]
        D = c.B[r0:r1, r0:r1].toarray()
        L = np.linalg.cholesky(D)
        c.A.append(D.astype(np.longdouble))
        c.M.append(np.abs(L) @ np.abs(L).T)
    return c


@pytest.mark.parametrize("wmax", BANDS)
def test_duplicated_band_blocks_at_the_edges(runs, wmax):
    import test_gpu_band_blocks as T
    on, off = runs
    c = _band_case(wmax)
    name = "band%d" % wmax
    s1 = on.i[name + ".stats"]
    assert s1["bj_max_bandwidth"] == max(w for _, w in c.blocks) and s1["bj_g4_bytes"] > 0
    # every shape is its own class: two members, and three of (17, .)
    assert s1["bj_paired_blocks"] == c.P - 1 and s1["bj_pair_tasks"] == len(ROWS) + 1, s1
    limit = np.array([(3 * w + 16) * U for _, w in c.blocks])
    for t in COLS:
        assert on.i["%s.paired%d" % (name, t)] == 1 and off.i["%s.paired%d" % (name, t)] == 0, t
        X = _panels(c.N, 500 + wmax)[t]
        Z1, Z0 = on.a["%s.Z%d" % (name, t)], off.a["%s.Z%d" % (name, t)]
        assert np.isfinite(Z1).all()
        om = T._omega(c, X, Z1)
        worst = int(np.argmax(om / limit))
        print("band %d t=%d: worst omega %.3f of the limit, block %d %s" % (wmax, t, om[worst] / limit[worst], worst, c.blocks[worst]))
        assert np.all(om <= limit), (wmax, t, worst, c.blocks[worst], om[worst], limit[worst])
        assert _same_bits(Z1, Z0), (wmax, t)


# ---- a refresh that splits a class -------------------------------------------------------------------------------------
def test_a_refresh_that_splits_a_class_falls_back_and_the_refresh_back_pairs_again(runs):
    on, off = runs
    st = {step: on.i["refresh." + step] for step in ("create", "doubled", "split", "back")}
    print("paired launch / shared blocks: " + ", ".join("%s %d / %d" % (k, s["bj_g4_last_paired"], s["bj_shared_blocks"]) for k, s in st.items()))
    assert st["create"]["bj_g4_last_paired"] == st["doubled"]["bj_g4_last_paired"] == st["back"]["bj_g4_last_paired"] == 1
    assert st["split"]["bj_g4_last_paired"] == 0
    assert st["split"]["bj_shared_blocks"] < st["create"]["bj_shared_blocks"] == st["back"]["bj_shared_blocks"]
    assert all(off.i["refresh." + step]["bj_g4_last_paired"] == 0 for step in st)
    for step in st:
        for t in COLS:
            key = "refresh.%s.Z%d" % (step, t)
            assert _same_bits(on.a[key], off.a[key]), key
    for t in COLS:
        assert _same_bits(on.a["refresh.back.Z%d" % t], on.a["refresh.doubled.Z%d" % t])
        assert not np.array_equal(on.a["refresh.split.Z%d" % t], on.a["refresh.doubled.Z%d" % t])
