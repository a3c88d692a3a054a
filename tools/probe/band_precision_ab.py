#!/usr/bin/env python3
"""In-process A/B of the storage of the one-copy band records (PREALPS_BJ_BAND_PRECISION: double / single) on the
headline workload (Q1 elasticity 70^3, boxes of 2 x 4 x 8 nodes = blocks of 192 rows): ONE operator; every window
creates the preconditioner in one precision, times APPLIES block solves of a t-column panel with the library's device
stopwatch (one k_bj_g4 launch each), solves to 1e-5 (preAlps_ECGSolve, host clock) and frees it.  The precisions
alternate (double first in even rounds).
usage: band_precision_ab.py [ROUNDS [T [N]]]     (defaults 5, 4, 70)
Prints one line per window, then median and minimum of every figure as one JSON line."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import prealps_amd as pa
from prealps_amd import gen
from prealps_amd.lib import check

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
t = int(sys.argv[2]) if len(sys.argv) > 2 else 4
n = int(sys.argv[3]) if len(sys.argv) > 3 else 70
applies = 50
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
L = prob.L
check(L.preAlps_hip_prepare_operator(t), "prepare")
rhs = prob.reference_rhs()
X = np.random.default_rng(0).standard_normal((prob.m, t))
dx, dy = prob.panel(t, t), prob.panel(t, t)
prob.to_device(dx, X, t)


def window(prec):
    prob.create_block_jacobi(band_precision=prec)
    assert prob.stat("bj_band_precision") == (32 if prec == "single" else 64)
    mb = prob.stat("bj_g4_bytes") / 1e6
    apply = lambda: check(L.preAlps_BlockJacobiApply(C.byref(dx), C.byref(dy)), "apply")
    for _ in range(5):
        apply()
    assert prob.stat("bj_g4_last_bits") == (32 if prec == "single" else 64)
    sec = C.c_double()
    check(L.preAlps_hip_timer_start(), "timer_start")
    for _ in range(applies):
        apply()
    check(L.preAlps_hip_timer_stop(C.byref(sec)), "timer_stop")
    r = prob.solve(rhs, t, tol=1e-5, max_iter=100000)
    L.preAlps_BlockJacobiFree()
    prob.has_precond = False
    return dict(prec=prec, apply_us=1e6 * sec.value / applies, records_MB=mb, iters=r.iters, solve_ms=1e3 * r.seconds,
                iter_us=1e6 * r.seconds / r.iters, final_res=r.final_res, ring=prob.stat("bj_g4_last_ring"))


window("double"); window("single")            # (first passes: allocations, plans, clocks)
res = {"double": [], "single": []}
for k in range(rounds):
    for prec in (("double", "single") if k % 2 == 0 else ("single", "double")):
        w = window(prec)
        res[prec].append(w)
        print("round %d  %-6s  k_bj_g4 %7.2f us  records %6.1f MB  %4d iterations to 1e-5  %8.2f ms  %7.2f us / iteration  (ring %d)"
              % (k, prec, w["apply_us"], w["records_MB"], w["iters"], w["solve_ms"], w["iter_us"], w["ring"]), flush=True)
keys = ("apply_us", "records_MB", "iters", "solve_ms", "iter_us")
summary = {"workload": "elasticity", "n": n, "nparts": int(P), "t": t, "rounds": rounds}
for p in res:
    for key in keys:
        vals = [w[key] for w in res[p]]
        summary["%s_%s_median" % (p, key)] = round(float(np.median(vals)), 3)
        summary["%s_%s_min" % (p, key)] = round(float(np.min(vals)), 3)
print(json.dumps(summary))
prob.panel_free(dx); prob.panel_free(dy)
prob.close()
