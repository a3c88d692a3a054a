"""The band block solve on synthetic blocks (gen.band_blocks_csr) placed on every dispatch edge, checked by the
componentwise backward error of every block.

Inputs.  Blocks L0 L0^T with prescribed rows b and a full band of exactly w, dense in values, optionally graded
(condition up to 7e6), shuffled (the library's RCM order, a non-identity row map) or coupled.  Blocks far below their
class maximum sit beside full-size ones; the class maxima sit on the edges of the dispatch: bands 32/33 .. 112/113
(the DQ of bj_g4_plan.c, the 4/6/8 tiles of k_bj_mfma, pa_bj_g4_max_band8, pa_bj_factor_wmax, pa_bj_g4_max_band), rows 192/193,
224/225, 256/257 (12/14/16 register tiles, then out of bj_g4), register classes at 64 k.

Criterion.  With B the scaled matrix (O.symrac_scale + O.permute_by_part), A_q = B[q, q], L its numpy Cholesky
factor, M = |L| |L|^T and r = X_q - A_q Z_q formed in np.longdouble,

    omega_q = max over rows and columns of |r| / (M |Z_q|).

A band Cholesky solve in precision u = 2^-53 has omega <= gamma ~ (3 (w + 1) + 1) u for any summation order (Higham,
Accuracy and Stability of Numerical Algorithms, Thm 10.4 with the band's w + 1 terms per inner product for n); the
records here are pre-scaled (L D^-1, D^-2, reciprocal pivots), a few more roundings per term:

    fp64 records:            omega_q <= (3 w_q + 16) u
    fp32 one-copy records:   omega_q <= 2^-23 * 1.01 + (3 w_q + 16) u      (the factor is rounded once, 2^-24 relative)

Neither depends on the conditioning.  w_q is the prescribed band; for a shuffled block the library's order has a band
that only bj_max_bandwidth bounds, and w_q = min(b_q - 1, bj_max_bandwidth) is used.  Every case also asserts a finite
output, identical bits from three more applies and, as a loose sanity bound only, a distance to the oracle's solve of
at most 1e3 cond_2(A_q) u per block in the Frobenius norm (fp32 records: 2^-24 for u).

Every case prints, per kernel family, its worst omega / limit beside the oracle's worst omega / limit on the same
blocks (lines "FAMILY ..."), and the classes it ran with the statistics that show which records exist (lines
"CLASSES ...").

PREALPS_BJ_G4_RING, PREALPS_BJ_G4_WIDE and PREALPS_BJ_GRAM are read once per process: the cases that set one of them
run in a child process that imports this module (one child per setting, under its own time limit); a child that was
killed fails the test and no further child is started."""
import contextlib
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
U = 2.0 ** -53
RTOL_HIST = 1e-8            # (test_gpu_configs.py / test_gpu_parity.py)
BASE_ENV = {"PREALPS_BJ_ND": "0"}
WAVEFRONT = {"PREALPS_BJ_WIDE_FROM": "448"}


# ---- the problems ---------------------------------------------------------------------------------------------
def _spread(blocks, seed):
    """A fixed shuffle of the block list, so that neighbours in a class list (the four blocks of a workgroup) differ
    in rows and band."""
    order = np.random.default_rng(seed).permutation(len(blocks))
    return [blocks[i] for i in order]


def _band_depth(wmax):
    """192 rows with bands wmax, wmax - 15, wmax - 16 and 5 -- those below the register class of wmax (64 k + 1 ..
    64 k + 64) raised to its first band -- beside 17 and 100 rows at wmax; every block twice."""
    lo = 1 if wmax <= 64 else 65
    ws = sorted({max(w, lo) for w in (wmax, wmax - 15, wmax - 16, 5)})
    return _spread(2 * ([(192, w) for w in ws] + [(17, wmax), (100, wmax)]), wmax)


def _row_edge(bmax):
    """bmax rows at bands 40 and 112 (register classes 2 and 3) beside 1, 2, 16 and 130 rows."""
    return _spread(2 * [(bmax, 40), (bmax, 112), (130, 40), (130, 112), (16, 40), (2, 1), (1, 0)], bmax)


def _main_class_last(blocks):
    """The library numbers the register classes by first appearance and launches them in that order: one block of
    every other class goes to the front, so that the class of the widest band is launched last and the statistics
    of the last launch (bj_g4_last_*) are its own."""
    cls = lambda bw: (min(bw[1], bw[0] - 1) + 127) // 64
    main = cls(max(blocks, key=lambda bw: min(bw[1], bw[0] - 1)))
    front, seen = [], {main}
    for i, bw in enumerate(blocks):
        if cls(bw) not in seen:
            seen.add(cls(bw))
            front.append(i)
    return [blocks[i] for i in front] + [bw for i, bw in enumerate(blocks) if i not in front]


MIXED_B = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192]
GRAM_B = [2, 3, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192]
GRAM_COUPLING = (1, 4.0)      # (the oracle needs 17 iterations; with (2, 0.05) it needs 7)

PROBLEMS = {
    "mixed": lambda: _spread([(b, w) for b in MIXED_B for w in (0, 5, 32, 33, 64)], 1),
    "outside": lambda: _spread([(b, w) for b in (257, 300) for w in (64, 65, 112)] +
                               [(192, w) for w in (113, 128, 129, 192, 193)] + [(300, 192), (300, 193)], 2),
    "wide": lambda: [(b, w) for w in (97, 256, 257, 448, 449) for b in (w + 1, 500)],
    "gram": lambda: _spread([(b, w) for b in GRAM_B for w in (1, 5, 32, 33, 64)], 3),
    "gram256": lambda: _spread(3 * [(256, 80), (256, 65), (200, 70), (130, 80), (100, 66), (70, 69), (66, 65)], 4),
    "gram256-76": lambda: _spread(3 * [(256, 76), (256, 65), (200, 70), (130, 76), (100, 66), (70, 69), (66, 65)], 5),
}
for _w in (32, 48, 49, 64, 80, 81, 96, 112):
    PROBLEMS["depth%d" % _w] = functools.partial(_band_depth, _w)
for _b in (193, 224, 225, 256):
    PROBLEMS["rows%d" % _b] = functools.partial(_row_edge, _b)
PROBLEMS["rows256-40"] = lambda: _spread(2 * [(256, 40), (256, 33), (130, 40), (16, 40), (2, 1), (1, 0)], 6)
PROBLEMS["rows256-28"] = lambda: _spread(2 * [(256, 28), (256, 17), (130, 28), (16, 40), (2, 1), (1, 0)], 7)


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name, grading=0.0, shuffle=False, coupled=False):
    """The matrix, the scaled and permuted B every test here compares with, and per block: A_q, M = |L| |L|^T,
    cond_2(A_q).  Built once and left unchanged."""
    from oracle import oracle as O
    from prealps_amd import gen
    c = _Case()
    c.name, c.grading, c.shuffle = name, grading, shuffle
    c.blocks = [(b, min(w, b - 1)) for b, w in _main_class_last(PROBLEMS[name]())]
    seed = 1000 + sorted(PROBLEMS).index(name)
    c.rp, c.ci, c.v, c.part, c.P = gen.band_blocks_csr(c.blocks, seed, grading=grading, shuffle=shuffle,
                                                       coupling=GRAM_COUPLING if coupled else None)
    c.N = len(c.rp) - 1
    A = sp.csr_matrix((c.v, c.ci, c.rp), shape=(c.N, c.N))
    c.B, perm, c.rowpos = O.permute_by_part(O.symrac_scale(A), c.part, c.P)
    assert np.array_equal(perm, np.arange(c.N))                       # (parts are contiguous: no permutation)
    c.A, c.M, c.cond = [], [], []
    for q in range(c.P):
        r0, r1 = c.rowpos[q], c.rowpos[q + 1]
        D = c.B[r0:r1, r0:r1].toarray()
        L = np.linalg.cholesky(D)
        c.A.append(D.astype(np.longdouble))
        c.M.append(np.abs(L) @ np.abs(L).T)
        c.cond.append(float(np.linalg.cond(D)))
    return c


def _omega(c, X, Z):
    """omega_q of every block."""
    om = np.empty(c.P)
    for q in range(c.P):
        r0, r1 = c.rowpos[q], c.rowpos[q + 1]
        r = np.abs(X[r0:r1].astype(np.longdouble) - c.A[q] @ Z[r0:r1].astype(np.longdouble)).astype(np.float64)
        den = c.M[q] @ np.abs(Z[r0:r1])
        zero = den == 0
        assert not np.any(r[zero] != 0)
        om[q] = float(np.max(r[~zero] / den[~zero])) if np.any(~zero) else 0.0
    return om


@functools.lru_cache(maxsize=None)
def _reference(name, grading, shuffle, t):
    """X (standard normal: every block sees every column), the oracle's solve and its omega_q: once per case and t."""
    from oracle import oracle as O
    c = _case(name, grading, shuffle)
    X = np.random.default_rng(100 * t + len(name)).standard_normal((c.N, t))
    Zo = np.ascontiguousarray(O.BlockJacobi(c.B, c.rowpos).apply(X))
    X.setflags(write=False)
    Zo.setflags(write=False)
    return X, Zo, _omega(c, X, Zo)


# ---- which kernel a class of blocks is given to (pa_bj_band_plan of bj_band_plan.c, pa_bj_layout_build; the labels of
# _family are checked against the planner in test_bj_band_plan_cpu.py) ------------------------------------------------
def _stride(t):
    ts = 2
    while ts < t:
        ts <<= 1
    return ts


def _classes(blocks, env):
    """[(R, wmax, bmax, [block ids])] in the library's order (classes by first appearance); R < 0: one workgroup
    per block (k_bj_wide)."""
    wide_from = 96 if len(blocks) < 1024 else 448
    if env.get("PREALPS_BJ_WIDE_FROM"):
        wide_from = min(max(int(env["PREALPS_BJ_WIDE_FROM"]), 96), 448)
    out = []
    for q, (b, w) in enumerate(blocks):
        R = (w + 127) // 64
        if w > wide_from:
            R = -1                                         # (windows above 1024 rows do not occur here)
        for cl in out:
            if cl[0] == R:
                break
        else:
            cl = [R, 0, 0, []]
            out.append(cl)
        cl[1], cl[2] = max(cl[1], w), max(cl[2], b)
        cl[3].append(q)
    return out


def _g4_class(cl, env):
    return env.get("PREALPS_BJ_G4", "1") != "0" and cl[0] > 0 and cl[1] <= 112 and cl[2] <= 256


def _family(cl, t, env, bits):
    R, wmax, bmax, _ = cl
    ts = _stride(t)
    if R < 0:
        return "k_bj_wide"
    g4_wide = env.get("PREALPS_BJ_G4_WIDE", "1") != "0"
    if _g4_class(cl, env) and (ts <= 4 or (ts == 8 and g4_wide and wmax <= 80)):
        return "k_bj_g4 %d tiles fp%d%s" % (16 if bmax > 224 else 14 if bmax > 192 else 12, bits,
                                             " two column sets" if ts == 8 else "")
    if wmax <= 112 and ts >= 8:
        return "k_bj_mfma %d tiles" % (4 if wmax <= 48 else 6 if wmax <= 80 else 8)
    if ts <= 4 and R in (2, 3):
        return "k_bj_apply_pairs"
    return "k_bj_apply R=%d" % R


def _g4_launch(cl, bits, ring_env, t):
    """(ring depth, pipelined) that the launch planner (bj_g4_plan.c) reports for the class: G4F_RING = 4 buffers on the pipelined chain."""
    wmax, bmax = cl[1], cl[2]
    cbuf = ((bits // 8) * (wmax + 4) + 127) & ~127
    nld = cbuf >> 7
    ring = ring_env if ring_env in (2, 4, 8) else 8        # (far fewer than two blocks per SIMD here)
    while ring > 2 and ((ring - 1) * nld > 15 or ring * cbuf * 8 > 40 * 1024):
        ring >>= 1
    dq = max(((wmax + 15) >> 4) + 1, 3)
    if bits == 64 and _stride(t) <= 4 and bmax <= 192 and dq <= 5 and ring >= 4:
        return 4, 1
    return ring, 0


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


# ---- one case ----------------------------------------------------------------------------------------------------
def run_apply(name, ts, grading=0.0, shuffle=False, precision=None, env=None, band_range=None):
    """Create the block solve of problem `name` under `env`, apply it to t columns for every t of ts and check
    every block.  band_range: the range bj_max_bandwidth has to stay in for a shuffled case.  Returns one record per
    t: the worst omega / limit per kernel family (kernel, oracle) and the statistics of the launch."""
    import prealps_amd
    env = dict(BASE_ENV, **(env or {}))
    c = _case(name, grading, shuffle)
    bits = 32 if precision == "single" else 64
    out = []
    with _environment(env):
        for k in ("PREALPS_BJ_G4_RING", "PREALPS_BJ_G4_WIDE", "PREALPS_BJ_GRAM"):
            assert env.get(k) == os.environ.get(k), "%s is read once per process: set it for a child" % k
        prob = prealps_amd.EcgProblem(c.rp, c.ci, c.v, c.P, c.part, scale=True, device=0)
        try:
            prob.create_block_jacobi(band_precision=precision)
            stats = {k: int(prob.stat(k)) for k in ("bj_max_bandwidth", "bj_g4_bytes", "bj_pairs_bytes",
                                                     "bj_band_precision", "bj_nd_blocks")}
            assert stats["bj_nd_blocks"] == 0
            assert np.array_equal(prob.rowpos, c.rowpos)
            if shuffle:
                lo, hi = band_range
                assert lo <= stats["bj_max_bandwidth"] <= hi, stats
                wlib = [min(b - 1, stats["bj_max_bandwidth"]) for b, w in c.blocks]
                # the classes of a shuffled case are not known block by block: one family, the intended one
                classes = [[(stats["bj_max_bandwidth"] + 127) // 64, stats["bj_max_bandwidth"], max(b for b, _ in c.blocks),
                            list(range(c.P))]]
            else:
                assert stats["bj_max_bandwidth"] == max(w for _, w in c.blocks), stats
                wlib = [w for _, w in c.blocks]
                classes = _classes(c.blocks, env)
                any_g4 = any(_g4_class(cl, env) for cl in classes)
                any_pairs = any(not _g4_class(cl, env) and cl[0] in (2, 3) for cl in classes)
                assert (stats["bj_g4_bytes"] > 0) == any_g4 and (stats["bj_pairs_bytes"] > 0) == any_pairs, stats
                assert stats["bj_band_precision"] == (bits if any_g4 else 0), stats
            limit = np.array([(3 * w + 16) * U for w in wlib]) + (2.0 ** -23 * 1.01 if bits == 32 else 0.0)
            for t in ts:
                X, Zo, om_o = _reference(name, grading, shuffle, t)
                Z = prob.block_jacobi_apply(X, t)
                launch = dict(ring=int(prob.stat("bj_g4_last_ring")), bits=int(prob.stat("bj_g4_last_bits")),
                              pipelined=int(prob.stat("bj_g4_last_pipelined")))
                again = all(_same_bits(Z, prob.block_jacobi_apply(X, t)) for _ in range(3))
                finite = bool(np.isfinite(Z).all())
                om = _omega(c, X, Z) if finite else np.full(c.P, np.inf)
                fwd = np.array([np.linalg.norm(Z[c.rowpos[q]:c.rowpos[q + 1]] - Zo[c.rowpos[q]:c.rowpos[q + 1]]) /
                                np.linalg.norm(Zo[c.rowpos[q]:c.rowpos[q + 1]]) for q in range(c.P)])
                fwd_limit = 1e3 * np.array(c.cond) * (2.0 ** -24 if bits == 32 else U)
                fam = {}
                for cl in classes:
                    f = _family(cl, t, env, bits if _g4_class(cl, env) else 64)
                    q = cl[3]
                    k = int(np.argmax(om[q] / limit[q]))
                    ko = int(np.argmax(om_o[q] / limit[q]))
                    e = fam.setdefault(f, dict(kernel=0.0, oracle=0.0, at=None, classes=[]))
                    e["classes"].append("R=%d wmax=%d bmax=%d n=%d" % (cl[0], cl[1], cl[2], len(q)))
                    if om[q][k] / limit[q][k] >= e["kernel"]:
                        e["kernel"], e["at"] = float(om[q][k] / limit[q][k]), list(c.blocks[q[k]])
                    e["oracle"] = max(e["oracle"], float(om_o[q][ko] / limit[q][ko]))
                tag = "%s%s%s%s t=%d %s" % (name, " graded %g" % grading if grading else "", " shuffled" if shuffle else "",
                                            " fp32" if bits == 32 else "", t,
                                            " ".join("%s=%s" % (k[11:], v) for k, v in sorted(env.items()) if k != "PREALPS_BJ_ND"))
                for f, e in sorted(fam.items()):
                    print("FAMILY %-38s | %-46s | kernel %.3f oracle %.3f of the limit, worst block %s"
                          % (f, tag, e["kernel"], e["oracle"], e["at"]))
                    print("CLASSES %s: %s -> %s; band %d, g4 %d B, pairs %d B, precision %d, last g4 launch %s, cond <= %.1e"
                          % (tag, "; ".join(e["classes"]), f, stats["bj_max_bandwidth"], stats["bj_g4_bytes"],
                             stats["bj_pairs_bytes"], stats["bj_band_precision"], launch, max(c.cond)))
                sys.stdout.flush()
                rec = dict(name=name, t=t, families=fam, launch=launch, stats=stats,
                           last_class=[classes[-1][1], classes[-1][2]],
                           last_g4=bool(_family(classes[-1], t, env, bits).startswith("k_bj_g4")))
                out.append(rec)
                assert finite, tag
                worst = int(np.argmax(om / limit))
                assert np.all(om <= limit), "%s: block %d %s has omega %.3e, limit %.3e (oracle %.3e)" % (
                    tag, worst, c.blocks[worst], om[worst], limit[worst], om_o[worst])
                assert again, "%s: repeated applies differ" % tag
                wf = int(np.argmax(fwd / fwd_limit))
                assert np.all(fwd <= fwd_limit), "%s: block %d %s is %.3e from the oracle, cond %.2e" % (
                    tag, wf, c.blocks[wf], fwd[wf], c.cond[wf])
        finally:
            prob.close()
    return out


def run_solve(name, env=None):
    """Orthodir t = 4, tol 1e-5 on the coupled problem `name`: the iteration count, the history and how many applies
    left the Gram block behind."""
    import prealps_amd
    env = dict(BASE_ENV, **WAVEFRONT, **(env or {}))
    c = _case(name, 0.0, False, True)
    with _environment(env):
        prob = prealps_amd.EcgProblem(c.rp, c.ci, c.v, c.P, c.part, scale=True, device=0)
        try:
            prob.create_block_jacobi()
            stats = {k: int(prob.stat(k)) for k in ("bj_max_bandwidth", "bj_g4_bytes", "bj_pairs_bytes", "bj_band_precision")}
            rhs = prob.reference_rhs()
            before = prob.stat("bj_gram_applies")
            got = prob.solve(rhs, 4, ortho_alg=prealps_amd.ORTHODIR, tol=1e-5, max_iter=1000)
            rec = dict(name=name, iters=int(got.iters), res=[float(r) for r in got.res], stats=stats,
                       gram_applies=int(prob.stat("bj_gram_applies") - before),
                       launch=dict(ring=int(prob.stat("bj_g4_last_ring")), bits=int(prob.stat("bj_g4_last_bits")),
                                   pipelined=int(prob.stat("bj_g4_last_pipelined"))))
        finally:
            prob.close()
    return rec


@functools.lru_cache(maxsize=None)
def _solve_reference(name):
    from oracle import oracle as O
    c = _case(name, 0.0, False, True)
    ref = O.ECG(c.B, c.rowpos, 4, O.ORTHODIR, O.NO_BS_RED, 1e-5, 1000).solve(O.reference_rhs(c.rowpos))
    return int(ref["iters"]), np.array(ref["res"])


def _check_solve(rec, gram, tag):
    """One class, on bj_g4; the oracle's iteration count (at least 15: the recurrence has run long enough for a
    wrong beta to show) and its history to RTOL_HIST."""
    c = _case(rec["name"], 0.0, False, True)
    classes = _classes(c.blocks, dict(BASE_ENV, **WAVEFRONT))
    iters, res = _solve_reference(rec["name"])
    d = np.abs(np.array(rec["res"][:len(res)]) - res[:len(rec["res"])]) / res[:len(rec["res"])]
    print("SOLVE %s %s: %d iterations (oracle %d), history within %.2e of the oracle's, %d applies left the Gram block, "
          "class R=%d wmax=%d bmax=%d, band %d, g4 %d B, pairs %d B, last g4 launch %s"
          % (rec["name"], tag, rec["iters"], iters, d.max(), rec["gram_applies"], classes[0][0], classes[0][1],
             classes[0][2], rec["stats"]["bj_max_bandwidth"], rec["stats"]["bj_g4_bytes"], rec["stats"]["bj_pairs_bytes"],
             rec["launch"]))
    assert len(classes) == 1 and _g4_class(classes[0], {})
    assert rec["stats"]["bj_g4_bytes"] > 0 and rec["stats"]["bj_pairs_bytes"] == 0
    assert rec["stats"]["bj_max_bandwidth"] == classes[0][1]
    assert iters >= 15
    assert rec["iters"] == iters
    assert len(rec["res"]) == len(res)
    np.testing.assert_allclose(rec["res"], res, rtol=RTOL_HIST)
    assert (rec["gram_applies"] > 0) == gram, rec["gram_applies"]
    assert rec["launch"]["bits"] == 64


# ---- children ------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import test_gpu_band_blocks as T
for job in json.loads(os.environ["BAND_BLOCKS_JOBS"]):
    fn = getattr(T, job.pop("fn"))
    for rec in (lambda r: r if isinstance(r, list) else [r])(fn(**job)):
        print("CASE " + json.dumps(rec), flush=True)
print("band blocks child ok")
"""


def _run_child(jobs, env, timeout=240):
    """One child under its own time limit; a child that was killed (signal or time limit) fails the test at once."""
    env = dict(os.environ, **BASE_ENV, **env)
    for j in jobs:                                            # what the child's run_apply / run_solve checks it runs under
        j["env"] = dict(j.get("env") or {}, **{k: v for k, v in env.items()
                                               if k in ("PREALPS_BJ_G4_RING", "PREALPS_BJ_G4_WIDE", "PREALPS_BJ_GRAM")})
    env["BAND_BLOCKS_JOBS"] = json.dumps(jobs)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT)], capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired as e:
        pytest.fail("child exceeded its time limit of %d s: %s" % (timeout, str(e.stderr or "")[-1500:]), pytrace=False)
    if r.returncode < 0:
        pytest.fail("child killed by signal %d: %s" % (-r.returncode, r.stderr[-2500:]), pytrace=False)
    print("".join(l + "\n" for l in r.stdout.splitlines() if l.startswith(("FAMILY", "CLASSES"))), end="")
    cases = [json.loads(l[5:]) for l in r.stdout.splitlines() if l.startswith("CASE ")]
    assert r.returncode == 0 and "band blocks child ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    return cases


def _families_of(recs):
    return {f for r in recs for f in r["families"]}


# ---- 1. mixed rows under the 12-tile build ----------------------------------------------------------------------
@pytest.mark.parametrize("grading", [0.0, 3.0])
def test_mixed_rows_on_the_one_copy_records(grading):
    """1 .. 192 rows x bands 0, 5, 32, 33, 64 in one launch of the 12-tile build (band 0: the class R = 1 beside
    it), t = 1 .. 4 on one column set, 8 on two (PREALPS_BJ_G4_WIDE unset = 1), 16 on k_bj_mfma."""
    recs = run_apply("mixed", [1, 2, 3, 4, 8, 16], grading=grading, env=WAVEFRONT)
    assert _families_of(recs) == {"k_bj_g4 12 tiles fp64", "k_bj_g4 12 tiles fp64 two column sets", "k_bj_mfma 4 tiles",
                                  "k_bj_mfma 6 tiles"}
    for r in recs:
        if r["t"] <= 4:            # few blocks, band <= 64: the pipelined chain
            assert r["launch"] == dict(ring=4, bits=64, pipelined=1), r["launch"]


@pytest.mark.parametrize("grading", [0.0, 3.0])
def test_mixed_rows_on_the_register_recurrences(grading):
    """PREALPS_BJ_G4=0: the same blocks through k_bj_apply_pairs (t <= 4, classes R = 2) and k_bj_apply (R = 1)."""
    recs = run_apply("mixed", [1, 2, 3, 4], grading=grading, env=dict(WAVEFRONT, PREALPS_BJ_G4="0"))
    assert _families_of(recs) == {"k_bj_apply_pairs", "k_bj_apply R=1"}
    assert all(r["stats"]["bj_g4_bytes"] == 0 and r["stats"]["bj_pairs_bytes"] > 0 for r in recs)


def test_mixed_rows_at_eight_columns_without_the_two_column_sets():
    """PREALPS_BJ_G4_WIDE=0 (a child): t = 8 stays with k_bj_mfma although the one-copy records exist."""
    recs = _run_child([dict(fn="run_apply", name="mixed", ts=[8], grading=g, env=WAVEFRONT) for g in (0.0, 3.0)],
                      {"PREALPS_BJ_G4_WIDE": "0"})
    assert len(recs) == 2 and _families_of(recs) == {"k_bj_mfma 4 tiles", "k_bj_mfma 6 tiles"}
    assert all(r["stats"]["bj_g4_bytes"] > 0 for r in recs)


def test_mixed_rows_shuffled():
    """A random symmetric permutation inside every block: the library's RCM order and a row map that is not the
    identity.  A full band of w <= 64 has an RCM band below 2 w: the one-copy records still take every class."""
    recs = run_apply("mixed", [4, 8], grading=3.0, shuffle=True, env=WAVEFRONT, band_range=(64, 112))
    assert all(r["stats"]["bj_g4_bytes"] > 0 and r["stats"]["bj_pairs_bytes"] == 0 for r in recs)


# ---- 2. one case per band depth -------------------------------------------------------------------------------------
@pytest.mark.parametrize("wmax", [32, 48, 64, 80, 96, 112])
def test_every_band_depth_of_the_one_copy_records(wmax):
    """The class maximum on the last band of each ring-buffer size of the launch planner (DQ = 3 .. 8 KiB), the other blocks
    15 and 16 below it and at the first band of the class; t = 4 for all, t = 8 on two column sets up to band 80
    (pa_bj_g4_max_band8) and on k_bj_mfma's 8 tiles above."""
    recs = run_apply("depth%d" % wmax, [4, 8], env=WAVEFRONT)
    want = {"k_bj_g4 12 tiles fp64", "k_bj_g4 12 tiles fp64 two column sets"}      # (above band 64 the 17 rows, band 16,
    if wmax > 80:                                                                  # are a class of their own)
        want.add("k_bj_mfma 8 tiles")
    assert _families_of(recs) == want


@pytest.mark.parametrize("wmax,t,tiles", [(81, 8, 8), (48, 16, 4), (49, 16, 6), (80, 16, 6), (81, 16, 8), (112, 16, 8)])
def test_every_tile_count_of_the_matrix_core_sweep(wmax, t, tiles):
    """k_bj_mfma on both sides of its 4 / 6 / 8-tile edges (bands 48 / 49, 80 / 81) and at its last band, 112."""
    recs = run_apply("depth%d" % wmax, [t], env=WAVEFRONT)
    want = {"k_bj_mfma %d tiles" % tiles}
    if wmax > 64:                   # the 17 rows (band 16) are in the register class below: a launch of their own
        want.add("k_bj_mfma 4 tiles" if t == 16 else "k_bj_g4 12 tiles fp64 two column sets")
    assert _families_of(recs) == want


# ---- 3. row edges of the tile builds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bmax,tiles", [(193, 14), (224, 14), (225, 16), (256, 16)])
def test_row_edges_of_the_tile_builds(bmax, tiles):
    """The largest block on the first and last row count of the 14- and 16-tile builds, at bands 40 and 112 (two
    classes), beside 1, 2, 16 and 130 rows.  256 rows is the largest index the packed row map holds."""
    recs = run_apply("rows%d" % bmax, [4, 8], env=WAVEFRONT)
    assert _families_of(recs) == {"k_bj_g4 12 tiles fp64", "k_bj_g4 %d tiles fp64" % tiles,                 # (band 0: R = 1)
                                  "k_bj_g4 12 tiles fp64 two column sets", "k_bj_g4 %d tiles fp64 two column sets" % tiles,
                                  "k_bj_mfma 8 tiles"}


@pytest.mark.parametrize("name,band_range", [("rows256-40", (40, 80)), ("rows256", (112, 112))])
def test_256_rows_shuffled(name, band_range):
    """Row-map entries of 255 away from the last tile: 256 rows at bands 40 and 33 (any RCM band up to 80 keeps both
    column sets on bj_g4), and at bands 40 and 112 (bj_g4 only if the order found has the band of the natural one)."""
    recs = run_apply(name, [4, 8], shuffle=True, env=WAVEFRONT, band_range=band_range)
    assert all(r["stats"]["bj_g4_bytes"] > 0 and r["stats"]["bj_pairs_bytes"] == 0 for r in recs)


# ---- 4. just outside bj_g4 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dispatch", ["wavefront", "default"])
def test_just_outside_the_one_copy_records(dispatch):
    """257 and 300 rows at bands 64, 65, 112; 192 rows at bands 113, 128, 129 and 191 (192 and 193 clipped); 300 rows
    at bands 192 and 193.  PREALPS_BJ_WIDE_FROM=448: register classes R = 2, 3 on k_bj_apply_pairs (t <= 4), R = 3 .. 5
    on k_bj_apply, R = 2 at t = 8 on k_bj_mfma; default (few blocks): bands above 96 on k_bj_wide."""
    recs = run_apply("outside", [2, 4, 8], env=WAVEFRONT if dispatch == "wavefront" else {})
    fams = _families_of(recs)
    assert all(r["stats"]["bj_g4_bytes"] == 0 for r in recs)
    if dispatch == "wavefront":
        assert fams == {"k_bj_apply_pairs", "k_bj_apply R=3", "k_bj_apply R=4", "k_bj_apply R=5", "k_bj_mfma 6 tiles"}
    else:
        assert fams == {"k_bj_apply_pairs", "k_bj_mfma 6 tiles", "k_bj_wide"}


# ---- 5. wide bands -------------------------------------------------------------------------------------------------------
def test_wide_bands():
    """Bands 97, 256, 257, 448, 449 in blocks of w + 1 and 500 rows, default dispatch: k_bj_factor_big and
    k_bj_layout_big factor them, k_bj_wide solves."""
    recs = run_apply("wide", [4, 16])
    assert _families_of(recs) == {"k_bj_wide"}


# ---- 6. fp32 records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rows256"])
def test_single_precision_records(name):
    recs = run_apply(name, [4, 8], precision="single", env=WAVEFRONT)
    assert all(r["stats"]["bj_band_precision"] == 32 for r in recs)
    assert any(f.startswith("k_bj_g4") and "fp32" in f for f in _families_of(recs))
    assert all(r["launch"]["bits"] == 32 and r["launch"]["pipelined"] == 0 for r in recs if r["last_g4"])


# ---- 7. ring depths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [2, 4, 8])
def test_ring_depths(ring):
    """PREALPS_BJ_G4_RING in a child: ring 2 is the memory-bound plain chain everywhere; 4 and 8 are the pipelined
    chain on the 12-tile build up to band 64 and the plain chain with as deep a ring as the LDS-DMA limit allows
    elsewhere: a chunk of band 80 or 112 is 6 or 8 LDS-DMA pieces and the ring stays at 2; 256 rows at band 40 are 3
    pieces, at most 4 buffers; at band 28 they are 2 pieces, and 8 buffers are allowed.  The class of the widest band
    is launched last (_main_class_last): what that launch reported is compared with the planner's rule (bj_g4_plan.c)."""
    jobs = [dict(fn="run_apply", name=n, ts=[4], grading=g, env=WAVEFRONT)
            for n, g in (("mixed", 3.0), ("depth80", 0.0), ("rows256", 0.0), ("rows256-40", 0.0), ("rows256-28", 0.0))]
    recs = _run_child(jobs, {"PREALPS_BJ_G4_RING": str(ring)})
    assert len(recs) == len(jobs)
    for r in recs:
        assert r["last_g4"]
        want = _g4_launch([0, r["last_class"][0], r["last_class"][1]], 64, ring, 4)
        print("ring %d %s: last class wmax %d bmax %d, launch %s" % (ring, r["name"], r["last_class"][0], r["last_class"][1], r["launch"]))
        assert (r["launch"]["ring"], r["launch"]["pipelined"]) == want, (r["name"], r["launch"], want)
        if ring == 2:
            assert r["launch"] == dict(ring=2, bits=64, pipelined=0)
    if ring > 2:
        got = {r["name"]: (r["launch"]["ring"], r["launch"]["pipelined"]) for r in recs}
        assert got == {"mixed": (4, 1), "depth80": (2, 0), "rows256": (2, 0), "rows256-40": (4, 0),
                       "rows256-28": (ring, 0)}, got


# ---- 8. factor on device = factor on host ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,grading", [("mixed", 3.0), ("depth112", 0.0)])
def test_host_factor_beside_the_device_factor(name, grading):
    """PREALPS_BJ_FACTOR=host against the default (k_bj_factor up to band 96, k_bj_factor_big above): both under the
    limit, and close to each other as two factorisations of the same blocks are."""
    dev = run_apply(name, [4], grading=grading, env=WAVEFRONT)
    host = run_apply(name, [4], grading=grading, env=dict(WAVEFRONT, PREALPS_BJ_FACTOR="host"))
    assert _families_of(dev) == _families_of(host)


# ---- 9. the Gram by-product on unequal blocks -------------------------------------------------------------------------------
def test_gram_by_product_on_unequal_blocks():
    """One class (bands 1 .. 64, 2 .. 192 rows) and nothing else, coupled so that Orthodir t = 4 needs at least 15
    iterations: the 4-column apply that leaves [in | prev]^T out behind, in the library's loop."""
    _check_solve(run_solve("gram"), True, "default")


@pytest.mark.parametrize("env", [{"PREALPS_BJ_GRAM": "0"}, {"PREALPS_BJ_G4_RING": "2"}, {"PREALPS_BJ_G4_RING": "4"}])
def test_gram_by_product_switches(env):
    (rec,) = _run_child([dict(fn="run_solve", name="gram")], env)
    _check_solve(rec, env.get("PREALPS_BJ_GRAM") != "0", json.dumps(env))
    want = dict(ring=2, bits=64, pipelined=0) if env.get("PREALPS_BJ_G4_RING") == "2" else dict(ring=4, bits=64, pipelined=1)
    assert rec["launch"] == want, rec["launch"]


@pytest.mark.parametrize("name,ring", [("gram256", 2), ("gram256-76", 4)])
def test_gram_by_product_on_the_plain_chain(name, ring):
    """Class maximum 256 rows: the 16-tile build, the plain (not pipelined) Gram chain.  At band 80 a chunk is six
    LDS-DMA pieces and the ring stays at 2; at band 76 it is five and the ring is 4 deep -- the depth at which the
    rows of the previous panel are loaded while older requests are still in flight."""
    rec = run_solve(name)
    _check_solve(rec, True, "default")
    assert rec["launch"] == dict(ring=ring, bits=64, pipelined=0), rec["launch"]
