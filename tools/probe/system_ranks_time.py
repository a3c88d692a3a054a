#!/usr/bin/env python3
"""What the caller's stopping metric costs per iteration where its sums ride on a collective: elasticity 70^3, boxes of
2 x 4 x 8 nodes, t = 4, ONE preAlps_hip_loopback shard (rank 3 of 8) in one process, so the iteration is the one of
several processes -- the halo pack, the riding launches, the lazy stopping test -- with empty collectives.
  solve_system on device tensors for a fixed number of iterations (tol = 0, max_iter = ITERS), stop="scaled" against
  stop="original", alternating over the rounds: microseconds per iteration.  The difference is the price of k_sys_norms
  and k_sys_norms_ride (start, gather, scatter and the final norms are in both).
There is no threshold: the yardstick is the scaled stop of the same process.
usage: system_ranks_time.py [ROUNDS [N [ITERS [OUT]]]]     (defaults 5, 70, 300, profiles/r18_system_ranks_time.txt)
Prints one line per variant and round and a JSON summary line, and writes both to OUT."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import prealps_amd as pa
from prealps_amd import gen

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 300
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r18_system_ranks_time.txt")
T, SHARD = 4, (3, 8)
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0, shard=SHARD)
prob.create_block_jacobi()
N = prob.N
b = np.random.default_rng(7).standard_normal(N)
tb = torch.from_numpy(b).to("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def system(stop):
    prob.sync()
    t0 = time.perf_counter()
    got = prob.solve_system(tb, T, stop=stop, tol=0.0, max_iter=iters)
    dt = time.perf_counter() - t0
    assert got.iters == iters, (stop, got.iters)
    return dict(seconds=dt, iterations=int(got.iters), us_per_iteration=round(1e6 * dt / iters, 2))


variants = ["scaled", "original"]
for stop in variants:      # (first passes: plan, row map, allocations, clocks)
    system(stop)
out = {stop: [] for stop in variants}
for r in range(rounds):
    for stop in (variants if r % 2 == 0 else variants[::-1]):
        rec = system(stop)
        out[stop].append(rec)
        say("round %d  stop=%-9s %s" % (r, stop, json.dumps(rec)))
med = {stop: float(np.median([x["us_per_iteration"] for x in out[stop]])) for stop in variants}
say(json.dumps({"n": n, "rows": N, "local_rows": prob.m, "halo_rows": prob.stat("halo_rows"), "shard": SHARD, "t": T,
                "rounds": rounds, "iterations_timed": iters, "us_per_iteration_scaled": round(med["scaled"], 2),
                "us_per_iteration_original": round(med["original"], 2),
                "us_per_iteration_difference": round(med["original"] - med["scaled"], 2)}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
prob.close()
