#!/usr/bin/env python3
"""What the caller's own system costs on the headline problem (elasticity 70^3, boxes of 2 x 4 x 8 nodes, t = 4, one
GPU), in ONE process, the variants alternating over the rounds:
  iteration: solve_system on device tensors for a fixed number of iterations (tol = 0, max_iter = ITERS), with
             stop="scaled" against stop="original": microseconds per iteration; the difference is the price of
             k_sys_norms and its finish (start, gather, scatter and the final norms are in both);
  around:    what surrounds the iteration, as wall seconds of a solve of 2 iterations: (a) today's way -- NumPy forms
             (d b)[perm], solve_multi, NumPy carries x back; (b) solve_system on host arrays; (c) solve_system on
             device tensors; and the NumPy permutation and scaling of (a) alone;
  to 1e-5:   iterations and seconds under each metric, and the relative residual ||b - A x|| / ||b|| recomputed on the
             host from the original CSR.
usage: system_solve_time.py [ROUNDS [N [ITERS]]]     (defaults 5, 70, 300)
Prints one line per variant and round and a JSON summary line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import scipy.sparse as sp
import torch
import prealps_amd as pa
from prealps_amd import gen

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 300
TOL, MAXIT, T = 1e-5, 5000, 4
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
prob.create_block_jacobi()
N = prob.N
A0 = sp.csr_matrix((v, ci, rp), shape=(N, N))
d, perm = prob.scaling, np.asarray(prob.perm)
b = np.random.default_rng(7).standard_normal(N)
tb = torch.from_numpy(b).to("cuda:0")


def todays_way(max_iter, tol):
    t0 = time.perf_counter()
    bl = (d * b)[perm]
    t1 = time.perf_counter()
    got = prob.solve(bl, T, tol=tol, max_iter=max_iter)
    t2 = time.perf_counter()
    x = np.empty(N)
    x[perm] = d[perm] * got.x
    t3 = time.perf_counter()
    return dict(seconds=t3 - t0, numpy_seconds=(t1 - t0) + (t3 - t2), iterations=int(got.iters), x=x)


def system(arg, stop, max_iter, tol):
    prob.sync()
    t0 = time.perf_counter()
    got = prob.solve_system(arg, T, stop=stop, tol=tol, max_iter=max_iter)
    dt = time.perf_counter() - t0
    return dict(seconds=dt, iterations=int(got.iters), x=got.x)


variants = {
    "iteration scaled (device, %d iterations)" % iters: lambda: system(tb, "scaled", iters, 0.0),
    "iteration original (device, %d iterations)" % iters: lambda: system(tb, "original", iters, 0.0),
    "around a: numpy + solve + numpy (2 iterations)": lambda: todays_way(2, 0.0),
    "around b: solve_system host arrays (2 iterations)": lambda: system(b, "scaled", 2, 0.0),
    "around c: solve_system device tensors (2 iterations)": lambda: system(tb, "scaled", 2, 0.0),
    "to 1e-5 scaled (device)": lambda: system(tb, "scaled", MAXIT, TOL),
    "to 1e-5 original (device)": lambda: system(tb, "original", MAXIT, TOL),
}
for f in variants.values():      # (first passes: plan, row map, allocations, clocks)
    f()
out = {name: [] for name in variants}
for r in range(rounds):
    order = list(variants) if r % 2 == 0 else list(variants)[::-1]
    for name in order:
        rec = variants[name]()
        x = rec.pop("x")
        if name.startswith("to 1e-5"):
            xh = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
            rec["true_relative_residual"] = float(np.linalg.norm(b - A0 @ xh) / np.linalg.norm(b))
        out[name].append(rec)
        print("round %d  %-56s %s" % (r, name, json.dumps(rec)), flush=True)


def med(name, key):
    return float(np.median([x[key] for x in out[name]]))


names = list(variants)
summary = {
    "us_per_iteration_scaled": round(1e6 * med(names[0], "seconds") / iters, 2),
    "us_per_iteration_original": round(1e6 * med(names[1], "seconds") / iters, 2),
    "around_ms": {k_: round(1e3 * med(k_, "seconds"), 3) for k_ in names[2:5]},
    "around_a_numpy_ms": round(1e3 * med(names[2], "numpy_seconds"), 3),
    "to_1e-5": {k_: dict(iterations=out[k_][0]["iterations"], median_seconds=round(med(k_, "seconds"), 6),
                         true_relative_residual=out[k_][0]["true_relative_residual"]) for k_ in names[5:]},
}
summary["us_per_iteration_difference"] = round(summary["us_per_iteration_original"] - summary["us_per_iteration_scaled"], 2)
print(json.dumps({"n": n, "rows": N, "rounds": rounds, "t": T, "iterations_timed": iters,
                  "system_map_bytes": prob.stat("op_system_map_bytes"), "summary": summary}))
prob.close()
