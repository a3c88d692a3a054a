#!/usr/bin/env python3
"""What the energy-norm estimate costs and what its stopping test buys: elasticity 70^3, boxes of 2 x 4 x 8 nodes, t = 4,
a random right-hand side, one process.  First on the whole problem, then on ONE preAlps_hip_loopback shard (rank 3 of 8:
the iteration of several processes -- halo pack, riding launches, lazy stopping test -- with empty collectives; its
iteration counts are those of the shard's own block, a rehearsal of the launches and not of the convergence).
  (a) solve_system on device tensors for a fixed number of iterations (tol = 0, max_iter = ITERS), stop="scaled" with
      energy=False against energy=True, alternating over the rounds: microseconds per iteration.  The difference is
      the price of k_energy_drops (one workgroup) and of the host's push into the tracker.
  (b) iterations and seconds to tol = 1e-5 under stop="scaled", "original" and "energy", alternating likewise, with
      the relative residual ||b - A x|| / ||b|| each leaves, formed on the host from the CSR arrays behind the timed
      region (whole problem only: a shard returns its own rows).
There is no threshold: the yardsticks are the other stops of the same process.  A loss is reported as it is.
usage: energy_stop_time.py [ROUNDS [N [ITERS [OUT]]]]     (defaults 5, 70, 300, profiles/r19_energy_stop_time.txt)
Prints one line per variant and round and a JSON summary line per setting, and writes all of it to OUT."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
import torch
import prealps_amd as pa
from prealps_amd import gen

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 300
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r19_energy_stop_time.txt")
T, SHARD, TOL, CAP = 4, (3, 8), 1e-5, 2000
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
A = sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def setting(shard):
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0, shard=shard)
    prob.create_block_jacobi()
    N = prob.N
    b = np.random.default_rng(7).standard_normal(N)
    tb = torch.from_numpy(b).to("cuda:0")
    name = "whole" if shard is None else "shard %d of %d" % shard

    def fixed(track):
        prob.sync()
        t0 = time.perf_counter()
        got = prob.solve_system(tb, T, stop="scaled", tol=0.0, max_iter=iters, energy=track)
        dt = time.perf_counter() - t0
        assert got.iters == iters, (track, got.iters)
        return dict(seconds=dt, iterations=int(got.iters), us_per_iteration=round(1e6 * dt / iters, 2))

    def to_tol(stop):
        prob.sync()
        t0 = time.perf_counter()
        got = prob.solve_system(tb, T, stop=stop, tol=TOL, max_iter=CAP)
        dt = time.perf_counter() - t0
        rec = dict(seconds=round(dt, 6), iterations=int(got.iters))
        if shard is None:      # (on the host: a library call at another width would make the next solve cut its plan anew)
            rec["true_relative_residual"] = float(np.linalg.norm(b - A @ got.x.cpu().numpy()) / np.linalg.norm(b))
        if stop == "energy":
            rec.update(relative_energy_error_estimate=float(got.err_est[0] / got.energy_norm[0]),
                       estimate_belongs_to_iteration=int(got.err_iter[0]))
        return rec

    tracks, stops = [False, True], ["scaled", "original", "energy"]
    for tr in tracks:      # (first passes: plan, row map, allocations, clocks)
        fixed(tr)
    for stop in stops:
        to_tol(stop)
    a = {tr: [] for tr in tracks}
    bb = {stop: [] for stop in stops}
    for r in range(rounds):
        for tr in (tracks if r % 2 == 0 else tracks[::-1]):
            rec = fixed(tr)
            a[tr].append(rec)
            say("%s  round %d  tracking=%-5s %s" % (name, r, tr, json.dumps(rec)))
        for stop in (stops if r % 2 == 0 else stops[::-1]):
            rec = to_tol(stop)
            bb[stop].append(rec)
            say("%s  round %d  stop=%-9s %s" % (name, r, stop, json.dumps(rec)))
    med = {tr: float(np.median([x["us_per_iteration"] for x in a[tr]])) for tr in tracks}
    summary = {"setting": name, "n": n, "rows": N, "local_rows": prob.m, "t": T, "rounds": rounds, "iterations_timed": iters,
               "us_per_iteration_untracked": round(med[False], 2), "us_per_iteration_tracked": round(med[True], 2),
               "us_per_iteration_difference": round(med[True] - med[False], 2), "tol": TOL}
    for stop in stops:
        summary[stop] = dict(iterations=bb[stop][0]["iterations"],
                             median_seconds=round(float(np.median([x["seconds"] for x in bb[stop]])), 6),
                             **{k: bb[stop][0][k] for k in bb[stop][0] if k not in ("seconds", "iterations")})
    say(json.dumps(summary))
    prob.close()


setting(None)
setting(SHARD)      # (last: the loopback hooks stay installed in the process)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
