#!/usr/bin/env python3
"""One process, the headline problem (elasticity 70^3, boxes of 2 x 4 x 8 nodes, t = 4), a random right-hand side, the
storage of the matrix values double / single in alternating rounds (EcgProblem.set_operator_precision: the fp32 copy
is formed or dropped inside the call, the fp64 array stays where it is).  Per round and storage:
  - the SpMM launch: REPS products on device panels between two events;
  - the iteration: an 800-iteration solve (tol 1e-30), wall seconds per iteration;
  - the bytes one product streams;
  - the caller's system to a TRUE 1e-5: solve_system(stop="original") at double against single with refine=True --
    iterations, passes, wall seconds and ||b - A x|| / ||b|| recomputed on the host from the original CSR.
usage: spmm_precision_time.py [ROUNDS [T [N]]]     (defaults 5, 4, 70)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import scipy.sparse as sp
import prealps_amd
from prealps_amd import gen
from prealps_amd.lib import check

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
t = int(sys.argv[2]) if len(sys.argv) > 2 else 4
n = int(sys.argv[3]) if len(sys.argv) > 3 else 70
REPS, TOL, MAX_ITER = 200, 1e-5, 4000

rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
N = len(rp) - 1
A0 = sp.csr_matrix((v, ci, rp), shape=(N, N))
prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
prob.create_block_jacobi()
L = prob.L
rng = np.random.default_rng(20261020)
b = rng.standard_normal(N)
rhs = prob.reference_rhs()
dx, dy = prob.panel(t, t), prob.panel(t, t)
prob.to_device(dx, rng.standard_normal((prob.m, t)), t)
prob.solve(rhs, t, tol=1e-30, max_iter=50)          # warm-up: plan, pools, clocks
print("elasticity %d^3: N = %d, nnz = %d, t = %d, %d rounds" % (n, N, rp[-1], t, rounds), flush=True)


def spmm_us():
    sec = C.c_double()
    for _ in range(10):
        check(L.preAlps_BlockOperator(C.byref(dx), C.byref(dy)), "preAlps_BlockOperator")
    check(L.preAlps_hip_timer_start(), "preAlps_hip_timer_start")
    for _ in range(REPS):
        check(L.preAlps_BlockOperator(C.byref(dx), C.byref(dy)), "preAlps_BlockOperator")
    check(L.preAlps_hip_timer_stop(C.byref(sec)), "preAlps_hip_timer_stop")
    return 1e6 * sec.value / REPS


for rnd in range(rounds):
    for precision in ("double", "single"):
        prob.set_operator_precision(precision)
        bits = int(prob.stat("spmm_precision"))
        us = spmm_us()
        prob.solve(rhs, t, tol=1e-30, max_iter=20)
        r = prob.solve(rhs, t, tol=1e-30, max_iter=800)
        print("round %d %-6s spmm_precision=%d: SpMM launch %.1f us, %.1f us per iteration (%d iterations), one product "
              "streams %.1f MB%s"
              % (rnd, precision, bits, us, 1e6 * r.seconds / r.iters, r.iters, prob.stat("spmm_precision_stream_bytes") / 1e6,
                 (" (fp32 copy %.1f MB, rounded in %.1f us)" % (prob.stat("spmm_val32_bytes") / 1e6,
                                                               1e6 * prob.stat("spmm_round_kernel_s")))
                 if prob.stat("spmm_val32_bytes") > 0 else ""), flush=True)
        kw = dict(refine=True) if precision == "single" else {}
        kw["max_iter"] = MAX_ITER
        prob.solve_system(b, t, stop="original", tol=TOL, **kw)                 # (pools and the row map: not timed)
        t0 = time.perf_counter()
        s = prob.solve_system(b, t, stop="original", tol=TOL, **kw)
        wall = time.perf_counter() - t0
        true = float(np.linalg.norm(b - A0 @ s.x) / np.linalg.norm(b))
        print("round %d %-6s solve_system%s: %d iterations%s, %.4f s wall, true ||b - A x|| / ||b|| = %.3e"
              % (rnd, precision, " + refine" if "refine" in kw else "", s.iters,
                 (", %d passes %s, %s" % (s.passes, s.pass_iters.tolist(), s.refine_status)) if "refine" in kw else "", wall, true),
              flush=True)
prob.panel_free(dx)
prob.panel_free(dy)
prob.close()
