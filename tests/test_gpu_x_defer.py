"""PREALPS_ECG_X_DEFER: the row pass of the solve-first iteration moves X every second time (k_update_xrz<4, skip / both>,
k_flush_x on a stop).  The additions to every x are those of the pass that moves X every time, in the same order, so
every output must be the same bytes with the switch off and on.  tests/test_gpu_solve_first.py's small problem; one
fresh child process per setting, each case in the same child."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(switch):
    env = dict(os.environ, PREALPS_ECG_X_DEFER=str(switch))
    for k in ("PREALPS_ECG_SOLVE_FIRST", "PREALPS_ECG_FUSE", "PREALPS_ECG_LAZY_NORM", "PREALPS_ECG_LAZY_STOP",
              "PREALPS_ECG_GRAPH", "PREALPS_BJ_GRAM", "PREALPS_RCI_FUSE", "PREALPS_ECG_POLL"):
        env.pop(k, None)
    return env


_CHILD = r"""
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

def counted(name, f):
    s0, f0, g0 = prob.stat("ecg_x_skips"), prob.stat("ecg_x_flushes"), prob.stat("bj_gram_applies")
    r = f()
    out["stat_" + name] = np.array([prob.stat("ecg_x_skips") - s0, prob.stat("ecg_x_flushes") - f0,
                                    prob.stat("bj_gram_applies") - g0])
    return r

# preAlps_ECGSolve to convergence, and stopped by max_iter on an owed update (7) and on none (8)
s = counted("solve", lambda: prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, bs_red=pa.NO_BS_RED, tol=1e-5, max_iter=1000))
out["solve_iters"] = np.array([s.iters]); out["solve_res"] = s.res; out["solve_x"] = s.x
for mi in (7, 8):
    r = counted("solve%%d" %% mi, lambda: prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, bs_red=pa.NO_BS_RED, tol=1e-5, max_iter=mi))
    out["solve%%d_iters" %% mi] = np.array([r.iters]); out["solve%%d_res" %% mi] = r.res; out["solve%%d_x" %% mi] = r.x

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

# preAlps_ECGAdvance in calls of (1, 1, 1), (2, 3) and (5, iters + 3, iters + 1) -- the last through two restarts -- with
# X and R read back after every call
for name, calls in (("a111", (1, 1, 1)), ("a23", (2, 3)), ("along", (5, int(s.iters) + 3, int(s.iters) + 1))):
    e, rci = start()
    for i, n in enumerate(calls):
        got = counted("%%s_%%d" %% (name, i), lambda: advance(e, rci, n))
        out["%%s_%%d_ret" %% (name, i)] = np.array(got); out["%%s_%%d_iter" %% (name, i)] = np.array([e.iter, e.res])
        out["%%s_%%d_X" %% (name, i)] = prob.to_host(e.X.contents, 4); out["%%s_%%d_R" %% (name, i)] = prob.to_host(e.R.contents, 4)
    out[name + "_x"] = finalize(e)
out["along_calls"] = np.array([5, int(s.iters) + 3, int(s.iters) + 1])

# a call that ends with the next iteration's product queued, then preAlps_ECGFinalize
e, rci = start()
counted("fin", lambda: advance(e, rci, 7))
out["fin_x"] = finalize(e)

# ... then the caller's own RCI loop for five iterations
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
out["rci_res"] = np.array(hist); out["rci_iter"] = np.array([e.iter]); out["rci_X"] = prob.to_host(e.X.contents, 4)
out["rci_x"] = finalize(e)

# preAlps_ECGSolveMulti (two systems), preAlps_ECGSolveGuess (one, from a guess), preAlps_ECGSolveSystem (the caller's units)
rng = np.random.default_rng(5)
B = np.asfortranarray(np.stack([rhs, rng.standard_normal(prob.m)], axis=1))
r = counted("multi", lambda: prob.solve_multi(B, 4, tol=1e-5, max_iter=1000))
out["multi_x"] = r.x; out["multi_res"] = r.res; out["multi_hist"] = r.sys_hist; out["multi_iters"] = np.array([r.iters])
x0 = 0.5 * s.x + 1e-3 * rng.standard_normal(prob.m)
r = counted("guess", lambda: prob.solve(rhs, 4, tol=1e-5, max_iter=1000, x0=x0))
out["guess_x"] = r.x; out["guess_res"] = r.res; out["guess_iters"] = np.array([r.iters])
b = rng.standard_normal(prob.N)
r = counted("system", lambda: prob.solve_system(b, 4, tol=1e-6, max_iter=1000))
out["system_x"] = r.x; out["system_res"] = r.res; out["system_hist"] = r.sys_hist; out["system_iters"] = np.array([r.iters])
prob.close()
np.savez(sys.argv[1], **out)
print("ok", int(s.iters))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("x_defer")
    script = tmp / "child.py"
    script.write_text(_CHILD % {"root": ROOT})
    res = {}
    for sw in (0, 1):
        f = str(tmp / ("x%d.npz" % sw))
        r = subprocess.run([sys.executable, str(script), f], capture_output=True, text=True, timeout=900, env=_env(sw),
                           cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res[sw] = dict(np.load(f))
    return res


def test_every_output_is_the_same_bytes(runs):
    a, b = runs[0], runs[1]
    assert sorted(a) == sorted(b)
    assert 8 < a["solve_iters"][0] < 1000 and a["solve7_iters"][0] == 7 and a["solve8_iters"][0] == 8
    assert sum(a["along_%d_ret" % i][0] for i in range(3)) >= 2                  # two restarts
    assert a["multi_iters"][0] > 2 and a["guess_iters"][0] > 2 and a["system_iters"][0] > 2
    for k in sorted(a):
        if k.startswith("stat_"):
            continue
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_the_switch_off_defers_nothing(runs):
    for k, v in runs[0].items():
        if k.startswith("stat_"):
            assert v[0] == 0 and v[1] == 0, (k, v)


def test_skips_and_flushes(runs):
    on = runs[1]
    # an unstopped call of n steps skips n // 2 times and flushes nothing
    for name, calls in (("a111", (1, 1, 1)), ("a23", (2, 3))):
        for i, n in enumerate(calls):
            assert tuple(on["stat_%s_%d" % (name, i)][:2]) == (n // 2, 0), (name, i)
    assert on["along_0_ret"][0] == 0 and tuple(on["stat_along_0"][:2]) == (5 // 2, 0)
    assert tuple(on["stat_fin"][:2]) == (7 // 2, 0)
    # a stop: at most one flush per stop, none without one (the calls through the restarts)
    for i in (1, 2):
        assert on["stat_along_%d" % i][1] <= on["along_%d_ret" % i][0]
    # preAlps_ECGSolve stopped by max_iter: 7 ends on an owed update, 8 does not
    assert tuple(on["stat_solve7"][:2]) == (4, 1) and tuple(on["stat_solve8"][:2]) == (4, 0)
    it = int(on["solve_iters"][0])
    assert tuple(on["stat_solve"][:2]) == ((it + 1) // 2, it % 2)


def test_the_solve_first_order_applied_to_several_systems_a_guess_and_a_system(runs):
    """X is deferred only inside solve_first_step, so the skips show that this order ran (the switch does not enter the
    choice of the order: the other child took the same one); a solve that stops after an odd number of steps flushes."""
    for name in ("multi", "guess", "system"):
        it = int(runs[1][name + "_iters"][0])
        assert tuple(runs[1]["stat_" + name][:2]) == ((it + 1) // 2, it % 2), name
        assert runs[1]["stat_" + name][2] == runs[0]["stat_" + name][2] > 0, name      # (the block solve left its Gram blocks)
