"""The host side of the solution history (prealps_amd/csrc/ecg_history.c) is plain host arithmetic: a stand-alone
program (tests/c/history_check.c) links the unit alone, is compiled with AddressSanitizer + UBSan and run as a program.
The ring, the Gram update and the scaled pivoted Cholesky are restated here, independently of the C code."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from history_ref import LD, U, gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
OK, BAD_ARGS, BAD_GRAM = 0, 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/history_check.c")
    tmp = tmp_path_factory.mktemp("ecg_history")
    out, unit = str(tmp / "history_check"), str(tmp / "ecg_history.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "ecg_history.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "history_check.c"), unit, "-o", out, "-lm"])
    return out


def run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    got = subprocess.run([exe], input=script, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert got.returncode == 0 and got.stderr == "", "sanitizer or program failure (%d):\n%s" % (got.returncode, got.stderr[-4000:])
    return [line.split() for line in got.stdout.splitlines()]


def hx(values):
    return " ".join("nan" if np.isnan(v) else float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel(order="F"))


def fl(words):
    return np.array([float("nan") if "nan" in w else float.fromhex(w) for w in words])


def test_the_unit_is_pure_host_arithmetic():
    src = open(os.path.join(CSRC, "ecg_history.c")).read() + open(os.path.join(CSRC, "ecg_history.h")).read()
    includes = sorted(set(line.split()[1] for line in src.splitlines() if line.startswith("#include")))
    assert includes == ['"ecg_history.h"', "<math.h>"]
    assert "getenv" not in src and "malloc" not in src and "static" not in src


class Ring:
    """The rule of the issue: a new column takes the next free slot; a full ring overwrites its oldest column."""

    def __init__(self, cap):
        self.cap, self.ids, self.slot_of = cap, [], {}       # ids: logical order, oldest first

    def push(self, ident):
        if len(self.ids) < self.cap:
            slot = len(self.ids)
        else:
            slot = self.slot_of.pop(self.ids.pop(0))
        self.ids.append(ident)
        self.slot_of[ident] = slot
        return slot


def _columns(rng, n, count):
    M = rng.standard_normal((n, n))
    return M @ M.T + n * np.eye(n), rng.standard_normal((n, count))


def append_script(ring, A, X, new_ids, dot):
    """The 'A' command for the columns new_ids, with the dots as the glue would form them: DO against the live
    columns by slot, DN among the new ones."""
    live = sorted(ring.slot_of.items(), key=lambda kv: kv[1])       # by slot: slots 0 .. count-1
    K, q = len(live), len(new_ids)
    DO = np.array([[dot(i, j) for j in new_ids] for i, _ in live]).reshape(K, q)
    DN = np.array([[dot(a, j) for j in new_ids] for a in new_ids])
    return "A %d %d %s %s\n" % (q, K, hx(DO), hx(DN))


@pytest.mark.parametrize("cap", [1, 2, 3, 16])
def test_ring_order_eviction_and_the_gram_of_the_survivors(exe, cap):
    rng = np.random.default_rng(100 + cap)
    sizes = [int(rng.integers(1, 6)) for _ in range(40)]
    A, X = _columns(rng, 7, sum(sizes))
    W = A @ X
    cache = {}

    def dot(i, j):      # x_i^T (A x_j), one value per ordered pair
        return cache.setdefault((i, j), float(X[:, i] @ W[:, j]))

    ring, script, expect, nxt = Ring(cap), "I %d\n" % cap, [], 0
    for q in sizes:
        ids = list(range(nxt, nxt + q))
        nxt += q
        script += append_script(ring, A, X, ids, dot) + "L\n"
        slots = [ring.push(i) if i in ids[-cap:] else -1 for i in ids]
        expect.append((ids, slots, list(ring.ids), dict(ring.slot_of)))
    out = run(exe, script)
    assert out[0] == ["I", "0"]
    for step, (ids, slots, order, slot_of) in enumerate(expect):
        a, g, l = out[1 + 3 * step], out[2 + 3 * step], out[3 + 3 * step]
        assert a[0] == "A" and int(a[1]) == OK and int(a[2]) == len(order), (step, a)
        assert [int(w) for w in a[4:]] == slots, (step, a, slots)
        assert [int(w) for w in l[1:1 + len(order)]] == [slot_of[i] for i in order], (step, l)
        assert l[-2:] == ["-1", "-1"]
        G = fl(g[1:]).reshape(16, 16)
        assert np.array_equal(G, G.T), step                       # symmetric in bits
        for i in order:
            for j in order:
                lo, hi = min(i, j), max(i, j)                      # the older column on the left
                assert G[slot_of[i], slot_of[j]] == dot(lo, hi), (step, i, j)
        dead = [s for s in range(16) if s not in slot_of.values()]
        assert not G[dead].any() and not G[:, dead].any()
    assert len(expect[-1][2]) == min(cap, sum(sizes))


@pytest.mark.parametrize("K,q", [(1, 1), (3, 2), (8, 4), (16, 16)])
def test_coefficients_and_backward_error(exe, K, q):
    rng = np.random.default_rng(7 * K + q)
    V = rng.standard_normal((K + 3, K))
    G = V.T @ V
    s = 1.0 / np.sqrt(np.diag(G))
    Gs = (G * s[:, None]) * s[None, :]
    Gs = np.triu(Gs, 1) + np.triu(Gs, 1).T + np.eye(K)
    gs = rng.standard_normal((K, q))
    out = run(exe, "S %d %d %s %s %s\n" % (K, q, float(1e-12).hex(), hx(Gs), hx(gs)))[0]
    rank = int(out[1])
    assert rank == K
    piv = [int(w) for w in out[2:2 + rank]]
    assert sorted(piv) == list(range(K)) and piv[0] == 0        # (equal pivots: the first)
    cs = fl(out[2 + rank:]).reshape(q, K).T
    ref = np.linalg.solve(Gs, gs)
    assert np.abs(cs - ref).max() <= 1e-10 * np.linalg.cond(Gs) * np.abs(ref).max()
    resid = np.abs(Gs.astype(LD) @ cs.astype(LD) - gs.astype(LD)).max(axis=0)
    bound = gamma(3 * K + 1) * K * np.abs(cs).astype(LD).sum(axis=0)
    assert (resid <= bound).all(), (resid, bound)


def _history_script(cap, A, X):
    W = A @ X
    ring, script = Ring(cap), "I %d\n" % cap
    for i in range(X.shape[1]):
        script += append_script(ring, A, X, [i], lambda a, b: float(X[:, a] @ W[:, b]))
        ring.push(i)
    return script


def _project(exe, cap, A, X, b, rtol=0.0):
    K = X.shape[1]
    out = run(exe, _history_script(cap, A, X) + "P 1 %s %s\n" % (float(rtol).hex(), hx(X.T @ b)))[-1]
    assert out[0] == "P"
    if int(out[1]) != OK:
        return int(out[1]), None, None, None
    vals = fl(out[3:])
    return OK, int(out[2]), vals[:K], vals[K]


def test_a_duplicate_and_a_zero_column_are_dropped(exe):
    rng = np.random.default_rng(5)
    A, X = _columns(rng, 9, 5)
    b = rng.standard_normal(9)
    st, rank, c4, cap4 = _project(exe, 8, A, X[:, :4], b)
    assert st == OK and rank == 4
    Xd = np.hstack([X[:, :4], X[:, 1:2]])                         # column 4 repeats column 1 exactly
    st, rank, c5, cap5 = _project(exe, 8, A, Xd, b)
    assert st == OK and rank == 4 and c5[4] == 0.0
    x4, x5 = X[:, :4] @ c4, Xd @ c5
    assert (np.abs(x5.astype(LD) - x4.astype(LD)) <= gamma(5) * (np.abs(Xd).astype(LD) @ np.abs(c5).astype(LD))).all()
    assert abs(cap5 - cap4) <= 16 * U * np.abs(c5 * (Xd.T @ b)).sum()
    Xz = np.hstack([X[:, :2], np.zeros((9, 1)), X[:, 2:4]])        # an all-zero column in the middle
    st, rank, cz, _ = _project(exe, 8, A, Xz, b)
    assert st == OK and rank == 4 and cz[2] == 0.0
    xz = Xz @ cz
    assert (np.abs(xz.astype(LD) - x4.astype(LD)) <= gamma(5) * (np.abs(Xz).astype(LD) @ np.abs(cz).astype(LD))).all()
    # captured = c^T g = ||x0||_A^2
    assert abs(cap4 - x4 @ A @ x4) <= 1e-10 * abs(cap4)
    # the threshold is an argument: a nearly dependent column is kept at 1e-12 and dropped at 1e-3
    Xn = np.hstack([X[:, :3], X[:, 1:2] + 1e-3 * X[:, 4:5]])
    assert _project(exe, 8, A, Xn, b)[1] == 4 and _project(exe, 8, A, Xn, b, rtol=1e-3)[1] == 3


def test_a_gram_matrix_that_is_not_finite_or_not_positive_is_refused(exe):
    rng = np.random.default_rng(6)
    A, X = _columns(rng, 6, 3)
    W = A @ X
    ring, script = Ring(4), "I 4\n"
    for i in range(3):
        dot = (lambda a, b: float("nan")) if i == 2 else (lambda a, b: float(X[:, a] @ W[:, b]))
        script += append_script(ring, A, X, [i], (lambda a, b, d=dot: d(a, b) if a != b else float(X[:, a] @ W[:, b])))
        ring.push(i)
    out = run(exe, script + "P 1 0x0p+0 %s\n" % hx(np.ones(3)))
    assert [int(r[1]) for r in out if r[0] == "A"] == [OK, OK, OK]      # (an off-diagonal NaN is the projection's to find)
    assert out[-1] == ["P", str(BAD_GRAM), "0"]
    # a diagonal entry that is not finite: the append itself refuses, and the ring is as it was
    out = run(exe, "I 2\nA 1 0 %s\nA 1 1 %s %s\nL\n" % (hx([2.0]), hx([1.0]), hx([np.inf])))
    assert out[1][:4] == ["A", "0", "1", "0"] and out[3][:4] == ["A", str(BAD_GRAM), "1", "0"]
    assert out[2] == out[4] and out[5] == ["L", "0", "|", "-1", "-1"]
    # only zero columns: no positive diagonal entry
    out = run(exe, "I 2\nA 1 0 %s\nP 1 0x0p+0 %s\n" % (hx([0.0]), hx([0.0])))
    assert out[-1] == ["P", str(BAD_GRAM), "0"]
    # an empty history: rank 0, no refusal
    assert run(exe, "I 3\nP 2 0x0p+0\n")[-1][:3] == ["P", "0", "0"]
