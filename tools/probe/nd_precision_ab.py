#!/usr/bin/env python3
"""In-process A/B of the storage of the sparse block factor (PREALPS_BJ_ND_PRECISION: double / single) on elasticity
70^3 with large blocks: ONE operator; every window creates the preconditioner in one precision, times APPLIES applies
of a t-column panel with the library's device stopwatch, solves to 1e-5 (preAlps_ECGSolve, host clock) and frees it.
The precisions alternate (double first in even rounds).
usage: nd_precision_ab.py [EDGE [ROUNDS [T]]]     (EDGE = subdomain edge in nodes: 18 -> 64 blocks of 17.5 k rows
(bench.py --full's survey_nparts), 35 -> 8 blocks of 128 k rows; defaults 18, 3, 4)
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

edge = int(sys.argv[1]) if len(sys.argv) > 1 else 18
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
t = int(sys.argv[3]) if len(sys.argv) > 3 else 4
applies = 20
rp, ci, v = gen.elasticity3d_csr(70)
part, P = gen.box_partition_nodes(70, (edge, edge, edge))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
L = prob.L
check(L.preAlps_hip_prepare_operator(t), "prepare")
rhs = prob.reference_rhs()
X = np.random.default_rng(0).standard_normal((prob.m, t))
dx, dy = prob.panel(t, t), prob.panel(t, t)
prob.to_device(dx, X, t)


def window(prec):
    t0 = time.perf_counter()
    prob.create_block_jacobi(nd_precision=prec)
    setup = time.perf_counter() - t0
    assert prob.stat("bj_nd_blocks") == P and prob.stat("bj_nd_precision") == (32 if prec == "single" else 64)
    gb = prob.stat("bj_factor_bytes") / 1e9
    apply = lambda: check(L.preAlps_BlockJacobiApply(C.byref(dx), C.byref(dy)), "apply")
    for _ in range(3):
        apply()
    sec = C.c_double()
    check(L.preAlps_hip_timer_start(), "timer_start")
    for _ in range(applies):
        apply()
    check(L.preAlps_hip_timer_stop(C.byref(sec)), "timer_stop")
    r = prob.solve(rhs, t, tol=1e-5, max_iter=100000)
    L.preAlps_BlockJacobiFree()
    prob.has_precond = False
    return dict(prec=prec, apply_ms=1e3 * sec.value / applies, factor_GB=gb, iters=r.iters, solve_s=r.seconds,
                it_per_s=r.iters / r.seconds, setup_s=setup, final_res=r.final_res)


window("double"); window("single")            # (first passes: allocations, plans, clocks)
res = {"double": [], "single": []}
for k in range(rounds):
    for prec in (("double", "single") if k % 2 == 0 else ("single", "double")):
        w = window(prec)
        res[prec].append(w)
        print("round %d  %-6s  apply %6.3f ms  factor %6.2f GB  %4d iterations to 1e-5  %.3f s  %6.1f it/s  (setup %.2f s)"
              % (k, prec, w["apply_ms"], w["factor_GB"], w["iters"], w["solve_s"], w["it_per_s"], w["setup_s"]), flush=True)
med = lambda p, key: round(float(np.median([w[key] for w in res[p]])), 4)
print(json.dumps({"edge": edge, "nparts": int(P), "rows_per_block": int(prob.m // P), "t": t, "rounds": rounds,
                  **{"%s_%s" % (p, key): med(p, key) for p in res for key in ("apply_ms", "factor_GB", "iters", "solve_s", "it_per_s")}}))
prob.panel_free(dx); prob.panel_free(dy)
prob.close()
