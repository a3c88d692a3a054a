"""PREALPS_ECG_SOLVE_FIRST: the library's own Orthodir loops with the block solve before the update (one finish and
one row pass per iteration) must give bitwise the results of the order of preAlps_ECGIterate.  Every setting runs in
a fresh child process; the two children's outputs are compared byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(switch):
    env = dict(os.environ, PREALPS_ECG_SOLVE_FIRST=str(switch))
    for k in ("PREALPS_ECG_FUSE", "PREALPS_ECG_LAZY_NORM", "PREALPS_ECG_LAZY_STOP", "PREALPS_ECG_GRAPH",
              "PREALPS_BJ_GRAM", "PREALPS_RCI_FUSE"):
        env.pop(k, None)
    return env


def _same_files(da, db):
    names = sorted(os.listdir(da))
    assert names and names == sorted(os.listdir(db)), (names, sorted(os.listdir(db)))
    for n in names:
        with open(os.path.join(da, n), "rb") as fa, open(os.path.join(db, n), "rb") as fb:
            assert fa.read() == fb.read(), "%s differs between the two orders" % n
    return names


def test_headline_dump_is_bitwise_identical(tmp_path):
    """bench.py's timed path (preAlps_ECGAdvance, 10 + 100 steps on the headline problem): X, R, x and the
    residual norm of both orders are the same files."""
    outs = {}
    for sw in (0, 1):
        d = str(tmp_path / ("sf%d" % sw))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100",
                            "--warmup", "10", "--dump-outputs", d], capture_output=True, text=True, timeout=1500,
                           env=_env(sw), cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[sw] = d
    names = _same_files(outs[0], outs[1])
    assert {"X.npy", "R.npy", "x.npy", "res.npy"} <= set(names), names


_SMALL = r"""
import sys, ctypes as C
sys.path.insert(0, %(root)r)
import numpy as np
import prealps_amd as pa
import prealps_amd.lib as pl
from prealps_amd import gen
from prealps_amd.lib import check
nn = (12, 10, 10)
rp, ci, v = gen.elasticity3d_csr(nn)
part, P = gen.box_partition_nodes(nn, (2, 2, 2))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
prob.create_block_jacobi()
L = prob.L
check(L.preAlps_hip_prepare_operator(4), "prepare")
rhs = np.ascontiguousarray(prob.reference_rhs())
prhs = rhs.ctypes.data_as(C.POINTER(C.c_double))
out = {}

# 1. preAlps_ECGSolve to convergence
s = prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, bs_red=pa.NO_BS_RED, tol=1e-5, max_iter=1000)
out["solve_iters"] = np.array([s.iters]); out["solve_res"] = s.res; out["solve_x"] = s.x

def start():
    e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, 1e-5, 1000)
    rci = C.c_int(0)
    check(L.preAlps_ECGInitialize(C.byref(e), prhs, C.byref(rci)), "init")
    check(L.preAlps_BlockJacobiApply(e.R, e.P), "apply")
    check(L.preAlps_BlockOperator(e.P, e.AP), "product")
    return e, rci

def advance(e, rci, n):
    rs, li, lr = C.c_int(0), C.c_int(0), C.c_double(0.0)
    check(L.preAlps_ECGAdvance(C.byref(e), prhs, C.byref(rci), n, C.byref(rs), C.byref(li), C.byref(lr)), "advance")
    return rs.value, li.value, lr.value

def finalize(e):
    x = np.zeros(prob.m)
    check(L.preAlps_ECGFinalize(C.byref(e), x.ctypes.data_as(C.POINTER(C.c_double))), "finalize")
    return x

# 2. preAlps_ECGAdvance through two stops and restarts, in three calls
e, rci = start()
got = [advance(e, rci, n) for n in (5, int(s.iters) + 3, int(s.iters) + 1)]
out["adv_restarts"] = np.array([g[0] for g in got]); out["adv_last_iters"] = np.array([g[1] for g in got])
out["adv_last_res"] = np.array([g[2] for g in got]); out["adv_iter"] = np.array([e.iter]); out["adv_res"] = np.array([e.res])
out["adv_X"] = prob.to_host(e.X.contents, 4); out["adv_R"] = prob.to_host(e.R.contents, 4)
out["adv_x"] = finalize(e)

# 3. a call that ends with the next iteration's product queued, then preAlps_ECGFinalize
e, rci = start()
advance(e, rci, 7)
out["fin_x"] = finalize(e)

# 4. ... then the caller's own RCI loop (examples/test_ecg_prealps_op.c:208-221) for five iterations
e, rci = start()
advance(e, rci, 7)
hist = []
for _ in range(5):
    stop = C.c_int(0)
    check(L.preAlps_ECGIterate(C.byref(e), C.byref(rci)), "iterate")
    check(L.preAlps_ECGStoppingCriterion(C.byref(e), C.byref(stop)), "stop")
    hist.append(e.res)
    check(L.preAlps_BlockJacobiApply(e.AP, e.Z), "apply")
    check(L.preAlps_ECGIterate(C.byref(e), C.byref(rci)), "iterate")
    check(L.preAlps_BlockOperator(e.P, e.AP), "product")
out["rci_res"] = np.array(hist); out["rci_iter"] = np.array([e.iter]); out["rci_x"] = finalize(e)
prob.close()
np.savez(sys.argv[1], **out)
print("ok", int(s.iters))
"""


def test_small_elasticity_solve_advance_restart_finalize(tmp_path):
    """A small elasticity problem that converges: preAlps_ECGSolve (iterations, residual history, solution),
    preAlps_ECGAdvance through stops and restarts in several calls, a call that ends with the next iteration's
    product queued followed by preAlps_ECGFinalize, and the caller's own RCI loop after such a call -- the same
    bytes in both orders."""
    script = tmp_path / "small.py"
    script.write_text(_SMALL % {"root": ROOT})
    res = {}
    for sw in (0, 1):
        f = str(tmp_path / ("small%d.npz" % sw))
        r = subprocess.run([sys.executable, str(script), f], capture_output=True, text=True, timeout=900,
                           env=_env(sw), cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res[sw] = dict(np.load(f))
    a, b = res[0], res[1]
    assert sorted(a) == sorted(b)
    assert a["solve_iters"][0] < 1000 and a["adv_restarts"].sum() >= 2, (a["solve_iters"], a["adv_restarts"])
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
