#!/usr/bin/env python3
"""What new values for the same pattern cost on the headline problem (elasticity 70^3, boxes of 2 x 4 x 8 nodes,
t = 4, one GPU), in ONE process, the two ways alternating over the rounds:
  update:   EcgProblem.update_values(v')  = preAlps_OperatorUpdateValues, host clock to the end of a device sync;
            its parts from preAlps_hip_get_stat: host (scaling vector + panel), the copy of the panel values to the
            device, the kernel (device seconds between two events, as preAlps_hip_timer_start / _stop take them);
            the first update, which cuts the value map of the plan, is reported apart from the later ones;
  rebuild:  preAlps_OperatorFree + preAlps_OperatorBuildFromCSR + preAlps_hip_prepare_operator(4), the only way
            without the entry, same clock.
The values alternate between v and v' = S v S, S = diag(1 + 0.3 (2u - 1)) (still SPD: a congruence), so every update
changes every value.  Then, once: iterations to 1e-5 on the updated operator with the factor of the old values kept
(lagged) and with the factor rebuilt, and the seconds of that rebuild.
usage: update_values_time.py [ROUNDS [N]]     (defaults 5, 70)
Prints one line per way and round and a JSON summary line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import prealps_amd as pa
from prealps_amd import gen

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
TOL, MAXIT, T = 1e-5, 5000, 4
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
N = len(rp) - 1
s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
v2 = s[np.repeat(np.arange(N), np.diff(rp))] * v * s[ci]
vals = (v, v2)


def build(values):
    t0 = time.perf_counter()
    p = pa.EcgProblem(rp, ci, values, P, part, scale=True, device=0)     # (frees the operator that stands)
    pa.lib.check(p.L.preAlps_hip_prepare_operator(T), "prepare")
    p.sync()
    return p, time.perf_counter() - t0


def update(p, values):
    p.sync()
    t0 = time.perf_counter()
    p.update_values(values)
    p.sync()
    dt = time.perf_counter() - t0
    return dt, {k: p.stat("op_update_%s_s" % k) for k in ("host", "copy", "kernel", "map")}


prob, first_build = build(v)
print("first build + plan                         %9.4f s" % first_build, flush=True)
dt, parts = update(prob, v2)
first = dict(seconds=dt, **parts)
print("first update (cuts the value map)          %9.4f s   map %.4f  host %.4f  copy %.4f  kernel %.6f"
      % (dt, parts["map"], parts["host"], parts["copy"], parts["kernel"]), flush=True)
map_bytes, stored = prob.stat("op_value_map_bytes"), prob.stat("spmm_stored_entries")
out = {"update": [], "rebuild": []}
which = 0                                  # v2 stands
for r in range(rounds):
    for way in (("update", "rebuild") if r % 2 == 0 else ("rebuild", "update")):
        which ^= 1
        if way == "update":
            if prob.stat("op_value_map_bytes") == 0:     # (after a rebuild: cut the map outside the clock)
                update(prob, vals[which ^ 1])
            dt, parts = update(prob, vals[which])
            out[way].append(dict(seconds=dt, **parts))
            print("round %d  update                            %9.4f s   host %.4f  copy %.4f  kernel %.6f"
                  % (r, dt, parts["host"], parts["copy"], parts["kernel"]), flush=True)
        else:
            prob, dt = build(vals[which])
            out[way].append(dict(seconds=dt, build=prob.stat("setup_build_s"), plan=prob.stat("setup_plan_s")))
            print("round %d  free + build + prepare            %9.4f s   build %.4f  plan %.4f"
                  % (r, dt, out[way][-1]["build"], out[way][-1]["plan"]), flush=True)

# iterations with the lagged and with the rebuilt factor: factor of v, operator of v2
prob, _ = build(v)
prob.create_block_jacobi()
b = np.random.default_rng(7).standard_normal(prob.m)
base = prob.solve(b, T, tol=TOL, max_iter=MAXIT)
prob.update_values(v2, precond="keep")
lagged = prob.solve(b, T, tol=TOL, max_iter=MAXIT)
t0 = time.perf_counter()
prob.update_values(v2, precond="rebuild")
prob.sync()
refactor = time.perf_counter() - t0
rebuilt = prob.solve(b, T, tol=TOL, max_iter=MAXIT)
print("solve to %.0e: %d iterations (%.4f s) on v; on v': %d (%.4f s) with the lagged factor, %d (%.4f s) with the "
      "rebuilt one; update + factor rebuild %.4f s"
      % (TOL, base.iters, base.seconds, lagged.iters, lagged.seconds, rebuilt.iters, rebuilt.seconds, refactor), flush=True)


def med(rows, key):
    return round(float(np.median([x[key] for x in rows])), 6)


summary = {"first_build_s": round(first_build, 6), "first_update": {k: round(x, 6) for k, x in first.items()},
           "update_median": {k: med(out["update"], k) for k in ("seconds", "host", "copy", "kernel")},
           "rebuild_median": {k: med(out["rebuild"], k) for k in ("seconds", "build", "plan")},
           "value_map_bytes": map_bytes, "stored_entries": stored,
           "iterations": {"old_values": int(base.iters), "lagged_factor": int(lagged.iters),
                          "rebuilt_factor": int(rebuilt.iters)},
           "solve_seconds": {"lagged_factor": round(lagged.seconds, 6), "rebuilt_factor": round(rebuilt.seconds, 6)},
           "update_plus_factor_rebuild_s": round(refactor, 6)}
print(json.dumps({"n": n, "rows": prob.m, "rounds": rounds, "tol": TOL, "t": T, "summary": summary}))
prob.close()
