#!/usr/bin/env python3
"""What the solution history costs and buys on a sequence of systems (elasticity n^3, t = 4, boxes of 2 x 4 x 8 nodes,
one GPU), in ONE process, cold and with a history of 8 alternating over the rounds:
  a 16-step sequence b_n = b_0 + (a slowly turning mix of four fixed random fields), solved to 1e-5 in the caller's
  units; per way and round the iterations and host seconds of every step;
  apart, the device time of project and of append (the library's stopwatch around REPS calls on device tensors, one
  column against a full ring of 8), which is what a step with history pays on top of its iterations.
usage: history_time.py [ROUNDS [N [STEPS]]]     (defaults 3, 70, 16)
Prints one line per way, round and step, and a JSON summary line."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import prealps_amd as pa
from prealps_amd import gen

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 16
TOL, MAXIT, T, CAP, REPS = 1e-5, 5000, 4, 8, 20
rp, ci, v = gen.elasticity3d_csr(n)
N = len(rp) - 1
part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
pa.lib.check(prob.L.preAlps_hip_prepare_operator(T), "prepare")
prob.create_block_jacobi()
prob.sync()
rng = np.random.default_rng(7)
base = rng.standard_normal(N)
fields = rng.standard_normal((N, 4))


def rhs(step):
    w = np.array([np.cos(0.2 * step), np.sin(0.2 * step), np.cos(0.1 * step + 1.0), np.sin(0.3 * step)])
    return base + fields @ w


def stopwatch(call):
    s = C.c_double()
    call()
    pa.lib.check(prob.L.preAlps_hip_timer_start(), "timer")
    for _ in range(REPS):
        call()
    pa.lib.check(prob.L.preAlps_hip_timer_stop(C.byref(s)), "timer")
    return s.value / REPS


out = {"cold": [], "history": []}
for r in range(rounds):
    for way in (("cold", "history") if r % 2 == 0 else ("history", "cold")):
        if way == "history":
            prob.enable_history(CAP)
        for step in range(1, steps + 1):
            got = prob.solve_system(rhs(step), T, tol=TOL, max_iter=MAXIT, history=way == "history")
            rec = dict(round=r, step=step, iters=got.iters, seconds=got.seconds,
                       rank=got.history_rank if way == "history" else 0)
            out[way].append(rec)
            print("round %d %-7s step %2d  %5d iterations  %8.4f s  rank %d" % (r, way, step, got.iters, got.seconds, rec["rank"]),
                  flush=True)
        if way == "history" and r == rounds - 1:
            import torch
            bd = torch.from_numpy(rhs(steps + 1)).cuda()
            xd = prob.history_project(bd)[0]
            project_s = stopwatch(lambda: prob.history_project(bd))
            append_s = stopwatch(lambda: prob.history_append(xd))
        if way == "history":
            prob.disable_history()
summary = dict(n=n, N=N, parts=P, t=T, tol=TOL, capacity=CAP, rounds=rounds, steps=steps,
               project_us=1e6 * project_s, append_us=1e6 * append_s)
for way in out:
    late = [x for x in out[way] if x["step"] > steps // 2]
    summary["%s_iters_per_step_late" % way] = float(np.mean([x["iters"] for x in late]))
    summary["%s_seconds_per_step_late" % way] = float(np.median([x["seconds"] for x in late]))
    summary["%s_iters_total" % way] = int(sum(x["iters"] for x in out[way]) // rounds)
print(json.dumps(summary))
prob.close()
