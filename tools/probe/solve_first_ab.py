#!/usr/bin/env python3
"""In-process A/B of PREALPS_ECG_SOLVE_FIRST (0: the order of preAlps_ECGIterate, 1: block solve before the update)
on the headline problem (elasticity 70^3, t = 4, one GPU): ONE EcgProblem and ONE solver object; every window sets
the switch, resets the solver (_preAlps_ECGReset reads it), runs a few untimed steps of preAlps_ECGAdvance -- the
path bench.py times -- and then times STEPS steps (host clock around the call and a sync, and the library's device
timer).  The SpMM's fast / slow mode is drawn per process, so only windows of one process compare.
usage: solve_first_ab.py [ROUNDS [STEPS]]     (defaults 8, 300; tol 1e-30: no stop inside a window)
Prints one line per window and a JSON summary line."""
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

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
warm = 20
rp, ci, v = gen.elasticity3d_csr(70)
part, P = gen.box_partition_nodes(70, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
prob.create_block_jacobi()
L = prob.L
check(L.preAlps_hip_prepare_operator(4), "prepare")
rhs = np.ascontiguousarray(prob.reference_rhs())
prhs = rhs.ctypes.data_as(C.POINTER(C.c_double))
e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, 1e-30, 10 ** 9)
rci = C.c_int(0)
check(L.preAlps_ECGInitialize(C.byref(e), prhs, C.byref(rci)), "ECGInitialize")


def advance(n):
    rs, li, lr = C.c_int(0), C.c_int(0), C.c_double(0.0)
    check(L.preAlps_ECGAdvance(C.byref(e), prhs, C.byref(rci), n, C.byref(rs), C.byref(li), C.byref(lr)), "advance")
    assert rs.value == 0, "a stop inside the window"


def window(sw):
    os.environ["PREALPS_ECG_SOLVE_FIRST"] = str(sw)
    check(L._preAlps_ECGReset(C.byref(e), prhs, C.byref(rci)), "reset")
    check(L.preAlps_BlockJacobiApply(e.R, e.P), "apply")
    check(L.preAlps_BlockOperator(e.P, e.AP), "product")
    advance(warm)
    prob.sync()
    dev = C.c_double()
    check(L.preAlps_hip_timer_start(), "timer_start")
    t0 = time.perf_counter()
    advance(steps)
    check(L.preAlps_hip_timer_stop(C.byref(dev)), "timer_stop")
    prob.sync()
    return 1e6 * (time.perf_counter() - t0) / steps, 1e6 * dev.value / steps, e.res


window(0); window(1)                 # (first passes: allocations, plans, clocks)
res = {0: [], 1: []}
for r in range(rounds):
    for sw in ((0, 1) if r % 2 == 0 else (1, 0)):
        host, dev, rn = window(sw)
        res[sw].append(host)
        print("round %d  SOLVE_FIRST=%d  %7.2f us/iteration (device timer %7.2f)  res %.17e" % (r, sw, host, dev, rn),
              flush=True)
a, b = np.array(res[0]), np.array(res[1])
print(json.dumps({"rounds": rounds, "steps": steps, "us_per_it_0": a.round(2).tolist(), "us_per_it_1": b.round(2).tolist(),
                  "median_0": round(float(np.median(a)), 2), "median_1": round(float(np.median(b)), 2),
                  "delta_median_us": round(float(np.median(b) - np.median(a)), 2),
                  "every_1_faster_than_every_0": bool(b.max() < a.min())}))
check(L.preAlps_ECGFinalize(C.byref(e), np.zeros(prob.m).ctypes.data_as(C.POINTER(C.c_double))), "finalize")
prob.close()
