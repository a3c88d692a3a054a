#!/usr/bin/env python3
"""What a start from an initial guess costs and gains on the headline problem (elasticity 70^3, boxes of 2 x 4 x 8
nodes, tol 1e-5, t = 4, one GPU), in ONE process, the variants alternating over the rounds:
  start:  preAlps_ECGInitializeMulti against preAlps_ECGInitializeGuess, host clock from the call to the end of a
          device sync, for one system (k = 1, s = 4) and for four (k = 4, s = 1); the solver is released untimed;
  solve:  (a) solve(b, 4) from zero, (b) solve(b, 4, x0 = the library's own tol = 1e-3 solution) -- iterations and
          seconds to 1e-5 (start and finish included), and the same pair for four systems, solve_multi(B, 4) against
          solve_multi(B, 4, X0 = its tol = 1e-3 solution).
usage: warm_start_time.py [ROUNDS [N]]     (defaults 5, 70)
Prints one line per variant and round and a JSON summary line."""
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
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
TOL, MAXIT, T = 1e-5, 5000, 4
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
prob.create_block_jacobi()
L, m = prob.L, prob.m
PD = C.POINTER(C.c_double)
B = np.asfortranarray(np.random.default_rng(7).standard_normal((m, 4)))
b = np.ascontiguousarray(B[:, 0])
check(L.preAlps_hip_prepare_operator(T), "prepare")
x3 = prob.solve(b, T, tol=1e-3, max_iter=MAXIT).x.copy()                    # (also the first pass: plan, clocks)
X3 = np.asfortranarray(prob.solve_multi(B, T, tol=1e-3, max_iter=MAXIT).x)
scratch = np.zeros((m, 4), order="F")


def start(k, guess):
    """Seconds of one initialise (to the end of a device sync); the solver is finalised outside the clock."""
    e = prob.new_ecg(T, pa.ORTHODIR, pa.NO_BS_RED, TOL, MAXIT)
    rci = C.c_int(0)
    rhs, x0 = B.ctypes.data_as(PD), X3.ctypes.data_as(PD)
    prob.sync()
    t0 = time.perf_counter()
    if guess:
        rc = L.preAlps_ECGInitializeGuess(C.byref(e), k, rhs, m, x0, m, C.byref(rci))
    else:
        rc = L.preAlps_ECGInitializeMulti(C.byref(e), k, rhs, m, C.byref(rci))
    prob.sync()
    dt = time.perf_counter() - t0
    check(rc, "initialise")
    check(L.preAlps_ECGFinalizeMulti(C.byref(e), scratch.ctypes.data_as(PD), m), "finalise")
    return dt


starts = {"start k=1 cold (InitializeMulti)": lambda: start(1, False),
          "start k=1 guess (InitializeGuess)": lambda: start(1, True),
          "start k=4 cold (InitializeMulti)": lambda: start(4, False),
          "start k=4 guess (InitializeGuess)": lambda: start(4, True)}
solves = {"a: solve(b, 4) from zero": lambda: prob.solve(b, T, tol=TOL, max_iter=MAXIT),
          "b: solve(b, 4, x0 = tol 1e-3 solution)": lambda: prob.solve(b, T, tol=TOL, max_iter=MAXIT, x0=x3),
          "c: solve_multi(B, 4) from zero": lambda: prob.solve_multi(B, T, tol=TOL, max_iter=MAXIT),
          "d: solve_multi(B, 4, X0 = tol 1e-3 solution)": lambda: prob.solve_multi(B, T, tol=TOL, max_iter=MAXIT, X0=X3)}
for f in list(starts.values()) + list(solves.values()):      # (first passes: allocations, clocks)
    f()
out_start = {name: [] for name in starts}
out_solve = {name: [] for name in solves}
for r in range(rounds):
    order = list(starts) if r % 2 == 0 else list(starts)[::-1]
    for name in order:
        dt = starts[name]()
        out_start[name].append(dt)
        print("round %d  %-46s %9.3f ms" % (r, name, 1e3 * dt), flush=True)
    order = list(solves) if r % 2 == 0 else list(solves)[::-1]
    for name in order:
        prob.sync()
        res = solves[name]()
        rec = dict(iterations=int(res.iters), seconds=round(res.seconds, 6))
        if res.sys_res0 is not None:
            rec["start_relative_residuals"] = (res.sys_res0 / res.sys_normb).tolist()
        out_solve[name].append(rec)
        print("round %d  %-46s %5d iterations  %.4f s to solution" % (r, name, res.iters, res.seconds), flush=True)
summary = {"start_median_ms": {k_: round(1e3 * float(np.median(v_)), 3) for k_, v_ in out_start.items()},
           "solve": {k_: dict(iterations=v_[0]["iterations"],
                              median_seconds=round(float(np.median([x["seconds"] for x in v_])), 6),
                              start_relative_residuals=v_[0].get("start_relative_residuals"))
                     for k_, v_ in out_solve.items()}}
print(json.dumps({"n": n, "rows": m, "rounds": rounds, "tol": TOL, "t": T, "summary": summary}))
prob.close()
