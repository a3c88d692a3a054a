#!/usr/bin/env python3
"""What several right-hand sides in one block iteration cost and gain on the headline problem (elasticity 70^3,
boxes of 2 x 4 x 8 nodes, tol 1e-5, one GPU), in ONE process, alternating three variants over four seeded
standard-normal right-hand sides:
  (a) four preAlps_ECGSolve calls, solve(b_j, 4);
  (b) one preAlps_ECGSolveMulti of the same four with t = 4 (s = 1);
  (c) the same with t = 8 (s = 2).
Per variant and round: iterations, seconds to solution (host clock around the calls, start and finish included) and
microseconds per iteration with the start and the finish taken off (the same call with max_iter = 1 is timed for
that, after one untimed call that takes the change of t: us/it = (seconds - seconds_1) / (iterations - calls)).
(b)'s iteration time against (a)'s is the cost of the per-system sums: the loop and the launches are otherwise the
same.
usage: multi_rhs_time.py [ROUNDS [N]]     (defaults 3, 70)
Prints one line per variant and round and a JSON summary line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import prealps_amd as pa
from prealps_amd import gen

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
TOL, MAXIT, K = 1e-5, 5000, 4
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
prob.create_block_jacobi()
B = np.asfortranarray(np.random.default_rng(7).standard_normal((prob.m, K)))
lrp, lci, lv = prob.local_csr()


def true_residuals(X):
    import scipy.sparse as sp
    A = sp.csr_matrix((lv, lci, lrp), shape=(prob.m, prob.M))
    return (np.linalg.norm(B - A @ X, axis=0) / np.linalg.norm(B, axis=0)).tolist()


def variant_a(max_iter):
    its, sec, X = 0, 0.0, np.zeros((prob.m, K))
    for j in range(K):
        r = prob.solve(np.ascontiguousarray(B[:, j]), 4, tol=TOL, max_iter=max_iter)
        its, sec, X[:, j] = its + r.iters, sec + r.seconds, r.x
    return its, sec, X, K


def variant_multi(t):
    def run(max_iter):
        r = prob.solve_multi(B, t, tol=TOL, max_iter=max_iter)
        return r.iters, r.seconds, r.x, 1
    return run


variants = {"a: 4 x solve(b_j, 4)": variant_a, "b: solve_multi(B, 4)": variant_multi(4),
            "c: solve_multi(B, 8)": variant_multi(8)}
for run in variants.values():            # (first passes: plans, allocations, clocks)
    run(3)
out = {name: [] for name in variants}
for r in range(rounds):
    names = list(variants) if r % 2 == 0 else list(variants)[::-1]
    for name in names:
        variants[name](1)                 # (takes the switch of the SpMM plan to this t off the timed calls)
        _, sec1, _, calls = variants[name](1)
        prob.sync()
        its, sec, X, calls = variants[name](MAXIT)
        us = 1e6 * (sec - sec1) / max(its - calls, 1)
        rec = dict(iterations=its, seconds=round(sec, 6), start_finish_seconds=round(sec1, 6), us_per_iteration=round(us, 2))
        if r == 0:
            rec["true_relative_residuals"] = true_residuals(X)
        out[name].append(rec)
        print("round %d  %-22s %5d iterations  %.4f s to solution  (start + finish %.4f s)  %8.2f us/iteration"
              % (r, name, its, sec, sec1, us), flush=True)
summary = {name: dict(iterations=v_[0]["iterations"],
                      median_seconds=round(float(np.median([x["seconds"] for x in v_])), 6),
                      median_us_per_iteration=round(float(np.median([x["us_per_iteration"] for x in v_])), 2),
                      true_relative_residuals=v_[0].get("true_relative_residuals"))
           for name, v_ in out.items()}
print(json.dumps({"n": n, "rows": prob.m, "rounds": rounds, "tol": TOL, "summary": summary}))
prob.close()
