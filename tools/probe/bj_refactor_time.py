#!/usr/bin/env python3
"""What a fresh block-Jacobi factor costs after new values on the headline problem (elasticity 70^3, 5670 boxes of
2 x 4 x 8 nodes, t = 4, one GPU), in ONE process, the two ways alternating over the rounds, host clock from the call
to the end of a device sync:
  rebuild:   EcgProblem.update_values(v', precond="rebuild")  = preAlps_OperatorUpdateValues + preAlps_BlockJacobiFree
             + preAlps_BlockJacobiCreate; of the create: setup_bj_factor_s (orders, band assembly on the host) and
             setup_bj_layout_s (uploads, device factorisation, layouts);
  refactor:  EcgProblem.update_values(v', precond="refactor") = preAlps_OperatorUpdateValues +
             preAlps_BlockJacobiUpdateValues; of the latter: bj_update_total_s, the copy of the panel values
             (bj_update_copy_s) and the device seconds of assembly + factorisation + second layouts
             (bj_update_kernel_s).  A create drops the band map, so after every rebuild the map is cut again by one
             refactor outside the clock; the cuts are reported apart (bj_update_map_s).
The values alternate between v and v' = S v S, S = diag(1 + 0.3 (2u - 1)) (still SPD: a congruence), so every call
changes every value.  Then: iterations to 1e-5 on v' with the factor of each way.
usage: bj_refactor_time.py [ROUNDS [N]]     (defaults 5, 70)
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

prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
pa.lib.check(prob.L.preAlps_hip_prepare_operator(T), "prepare")
t0 = time.perf_counter()
prob.create_block_jacobi()
prob.sync()
print("%d blocks, first create %.4f s (factor %.4f, layout %.4f); factor %.0f + one-copy records %.0f bytes"
      % (P, time.perf_counter() - t0, prob.stat("setup_bj_factor_s"), prob.stat("setup_bj_layout_s"),
         prob.stat("bj_factor_bytes"), prob.stat("bj_g4_bytes")), flush=True)
b = np.random.default_rng(7).standard_normal(prob.m)


def timed(values, way):
    prob.sync()
    t0 = time.perf_counter()
    prob.update_values(values, precond=way)
    prob.sync()
    dt = time.perf_counter() - t0
    keys = (("setup_bj_factor_s", "setup_bj_layout_s") if way == "rebuild" else
            ("bj_update_total_s", "bj_update_copy_s", "bj_update_kernel_s", "bj_update_map_s"))
    return dict(seconds=dt, op_host=prob.stat("op_update_host_s"), op_copy=prob.stat("op_update_copy_s"),
                **{k: prob.stat(k) for k in keys})


out = {"rebuild": [], "refactor": []}
cuts = []
which = 0                                  # v stands
for r in range(rounds):
    for way in (("rebuild", "refactor") if r % 2 == 0 else ("refactor", "rebuild")):
        if way == "refactor" and prob.stat("bj_band_map_bytes") == 0:      # (after a create: cut the map outside the clock)
            which ^= 1
            cuts.append(timed(vals[which], "refactor"))
            print("         refactor that cuts the band map   %9.4f s   map %.4f  (refactorisation %.4f: copy %.4f  kernels %.6f)"
                  % (cuts[-1]["seconds"], cuts[-1]["bj_update_map_s"], cuts[-1]["bj_update_total_s"],
                     cuts[-1]["bj_update_copy_s"], cuts[-1]["bj_update_kernel_s"]), flush=True)
        which ^= 1
        x = timed(vals[which], way)
        out[way].append(x)
        if way == "rebuild":
            print("round %d  update + free + create            %9.4f s   operator %.4f  create: factor %.4f  layout %.4f"
                  % (r, x["seconds"], x["op_host"] + x["op_copy"], x["setup_bj_factor_s"], x["setup_bj_layout_s"]), flush=True)
        else:
            print("round %d  update + refactor in place        %9.4f s   operator %.4f  refactorisation %.4f: copy %.4f  kernels %.6f"
                  % (r, x["seconds"], x["op_host"] + x["op_copy"], x["bj_update_total_s"], x["bj_update_copy_s"],
                     x["bj_update_kernel_s"]), flush=True)
map_bytes, map_entries = prob.stat("bj_band_map_bytes"), prob.stat("bj_band_map_entries")
factor_bytes, g4_bytes = prob.stat("bj_factor_bytes"), prob.stat("bj_g4_bytes")

# iterations on v' with the factor of each way
prob.update_values(v, precond="rebuild")
prob.update_values(v2, precond="rebuild")
rebuilt = prob.solve(b, T, tol=TOL, max_iter=MAXIT)
prob.update_values(v, precond="refactor")
prob.update_values(v2, precond="refactor")
refreshed = prob.solve(b, T, tol=TOL, max_iter=MAXIT)
same = bool(np.array_equal(rebuilt.x.view(np.uint64), refreshed.x.view(np.uint64)))
print("solve to %.0e on v': %d iterations (%.4f s) with the rebuilt factor, %d (%.4f s) with the factor refreshed in "
      "place; x bitwise equal: %s" % (TOL, rebuilt.iters, rebuilt.seconds, refreshed.iters, refreshed.seconds, same), flush=True)
print("band map: %.0f entries, %.0f bytes; plain records %.0f bytes, one-copy records %.0f bytes"
      % (map_entries, map_bytes, factor_bytes, g4_bytes), flush=True)


def med(rows, key):
    return round(float(np.median([x[key] for x in rows])), 6)


summary = {"rebuild_median": {k: med(out["rebuild"], k) for k in ("seconds", "setup_bj_factor_s", "setup_bj_layout_s")},
           "refactor_median": {k: med(out["refactor"], k) for k in ("seconds", "bj_update_total_s", "bj_update_copy_s",
                                                                    "bj_update_kernel_s")},
           "map_cut_median": {k: med(cuts, k) for k in ("seconds", "bj_update_map_s")} if cuts else None,
           "band_map_bytes": map_bytes, "band_map_entries": map_entries, "bj_factor_bytes": factor_bytes,
           "bj_g4_bytes": g4_bytes,
           "iterations": {"rebuilt_factor": int(rebuilt.iters), "refreshed_factor": int(refreshed.iters)},
           "x_bitwise_equal": same}
print(json.dumps({"n": n, "rows": prob.m, "blocks": P, "rounds": rounds, "tol": TOL, "t": T, "summary": summary}))
prob.close()
