#!/usr/bin/env python3
"""What the entries of the solution history cost on a shard, where a row panel is an eighth of the problem and an iteration
is short: elasticity 70^3, boxes of 2 x 4 x 8 nodes, t = 4, ONE preAlps_hip_loopback shard (rank 3 of 8, the shard of
tools/probe/system_ranks_time.py) in one process.  The shard's collectives are empty and its halo rows arrive as zeros: the
probe rehearses the launches, allocations and drains of a rank, not convergence, and no network.
  project   history_project of one column (a device tensor) against a full ring of 8
  append    history_append of one column (a device tensor) to that ring
  iteration solve_system on device tensors for ITERS iterations (tol = 0), per iteration
alternating over the rounds.  Each entry is timed twice: on the host around the call (every entry drains the stream
before it returns) and by two events on the library's stream.  Once, outside the timed rounds, torch's profiler lists the
kernels and memory operations each entry queues.
There is no threshold: the question is whether the entries' fixed costs (the temporary solver's allocation, the drains)
rather than their bytes decide on a shard.
usage: history_ranks_time.py [ROUNDS [N [ITERS [OUT]]]]     (defaults 5, 70, 300, profiles/r21_history_ranks_time.txt)
Prints one line per measurement and a JSON summary line, and writes both to OUT."""
import json
import os
import re
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
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r21_history_ranks_time.txt")
T, SHARD, RING = 4, (3, 8), 8
rp, ci, v = gen.elasticity3d_csr(n)
part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0, shard=SHARD)
prob.create_block_jacobi()
N = prob.N
rng = np.random.default_rng(7)
tb = torch.from_numpy(rng.standard_normal(N)).to("cuda:0")
tx = torch.from_numpy(rng.standard_normal((RING + 1, N))).to("cuda:0").t()      # strides (1, N)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


stream = torch.cuda.ExternalStream(int(prob.L.preAlps_hip_get_stream() or 0))


def timed(fn):
    prob.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    e1.record(stream)
    e1.synchronize()
    return out, 1e6 * dt, 1e3 * e0.elapsed_time(e1)


def project():
    return timed(lambda: prob.history_project(tb))


def append():
    return timed(lambda: prob.history_append(tx[:, RING]))


def iteration():
    got, host, dev = timed(lambda: prob.solve_system(tb, T, stop="original", tol=0.0, max_iter=iters))
    assert got.iters == iters, got.iters
    return got, host / iters, dev / iters


prob.enable_history(RING)
prob.history_append(tx[:, :RING])
assert prob.stat("hist_columns") == RING
variants = {"project": project, "append": append, "iteration": iteration}
for fn in variants.values():      # (first passes: plan, row map, allocations, clocks)
    fn()
out = {name: [] for name in variants}
order = list(variants)
for r in range(rounds):
    for name in (order if r % 2 == 0 else order[::-1]):
        _, host, dev = variants[name]()
        out[name].append((host, dev))
        say("round %d  %-9s host %.1f us, stream %.1f us%s" % (r, name, host, dev, " per iteration" if name == "iteration" else ""))
assert prob.stat("hist_columns") == RING

# what each entry queues, from torch's profiler (once, not timed)
queued = {}
try:
    from torch.profiler import ProfilerActivity, profile
    for name, fn in (("project", lambda: prob.history_project(tb)), ("append", lambda: prob.history_append(tx[:, RING]))):
        prob.sync()
        with profile(activities=[ProfilerActivity.CUDA]) as pf:
            fn()
            prob.sync()
        names = {}
        for ev in pf.events():
            if str(ev.device_type).endswith("CUDA"):
                found = re.search(r"\bk_\w+", ev.name)          # (the library's kernels; copies and fills by their own name)
                key = found.group(0) if found else ev.name.strip()
                names[key] = names.get(key, 0) + 1
        queued[name] = names
        say("%s queues %d device operations: %s" % (name, sum(names.values()), json.dumps(names, sort_keys=True)))
except Exception as e:      # (a build of torch without the tracer: the times stand without the list)
    say("the profiler is not available here (%s): no list of launches" % (e,))

med = {name: [float(np.median([x[i] for x in out[name]])) for i in (0, 1)] for name in variants}
say(json.dumps({"n": n, "rows": N, "local_rows": prob.m, "halo_rows": prob.stat("halo_rows"), "shard": SHARD, "t": T,
                "ring": RING, "rounds": rounds, "iterations_timed": iters,
                "project_us_host": round(med["project"][0], 1), "project_us_stream": round(med["project"][1], 1),
                "append_us_host": round(med["append"][0], 1), "append_us_stream": round(med["append"][1], 1),
                "iteration_us_host": round(med["iteration"][0], 2), "iteration_us_stream": round(med["iteration"][1], 2),
                "project_plus_append_in_iterations": round((med["project"][0] + med["append"][0]) / med["iteration"][0], 1),
                "device_operations": {k: sum(v_.values()) for k, v_ in queued.items()}}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
prob.disable_history()
prob.close()
