#!/usr/bin/env python3
"""What the coarse correction of the two-level block-Jacobi preconditioner costs and buys (elasticity, t = 4, the three
translations, default aggregates, one GPU), in ONE process, with and without the coarse space alternating over the
rounds -- the yardstick is the plain block-Jacobi solve of the same process:
  per round and way: iterations and host seconds of solve() to 1e-5 (random right-hand side, the same every round),
  microseconds per iteration; device seconds per preAlps_BlockJacobiApply from the library's stopwatch over REPS
  applies of a 4-column panel -- the difference of the two ways is the device time of the coarse stages together
  (k_coarse_restrict, k_coarse_gather + k_coarse_einv, k_coarse_prolong_add); bj_coarse_setup_s of every attach.
usage: coarse_space_time.py [ROUNDS [N [boxes|kway64]]]     (defaults 5, 70, boxes)
       coarse_space_time.py cap [THREADS ...]                (default 16 1; needs gcc, no GPU)
  boxes:  boxes of 2 x 4 x 8 nodes (70^3: 5670 parts; at the cap of 1536 unknowns that is 512 aggregates)
  kway64: 64 parts from the library's partitioner (one aggregate per part fits: 192 unknowns)
  cap:    the host set-up alone at the cap PA_COARSE_MAX_DOFS: coarse_space.c and tests/c/coarse_space_check.c are
          compiled with gcc -O2 -fopenmp into a temporary directory and run on Poisson 24^3 in as many contiguous
          parts as the cap holds, one constant vector, one aggregate per part, with OMP_NUM_THREADS = THREADS; the
          seconds are those of pa_coarse_build (chunk lists, E, Cholesky, explicit inverse).
Prints one line per way and round and a JSON summary line."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import prealps_amd as pa
from prealps_amd import gen, nearkernel



def cap_setup(threads):
    import re
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    csrc = os.path.join(root, "prealps_amd", "csrc")
    cap = int(re.search(r"#define\s+PA_COARSE_MAX_DOFS\s+(\d+)", open(os.path.join(csrc, "coarse_space.h")).read()).group(1))
    from prealps_amd import gen as g
    n = 24
    rp, ci, v = g.poisson3d_csr(n)
    N = n ** 3
    rowpos = (np.arange(cap + 1, dtype=np.int64) * N // cap).astype(np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, x) for x in ("check", "cap.in", "cap.out"))
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fopenmp", "-I", csrc, os.path.join(root, "tests", "c", "coarse_space_check.c"),
                               os.path.join(csrc, "coarse_space.c"), "-o", exe, "-lm"])
        with open(fin, "wb") as f:
            np.array([N, cap, 1, cap, 0, 0, len(v)], dtype=np.int32).tofile(f)
            rp.tofile(f); ci.tofile(f); v.tofile(f); rowpos.tofile(f)
            np.arange(cap, dtype=np.int32).tofile(f)
            np.ones((N, 1)).tofile(f)
        for th in threads:
            out = subprocess.run([exe, fin, fout], env=dict(os.environ, OMP_NUM_THREADS=str(th)), capture_output=True, text=True)
            print("cap %d unknowns, %2d threads: %s" % (cap, th, out.stdout.strip()), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "cap":
    cap_setup([int(x) for x in sys.argv[2:]] or [16, 1])
    sys.exit(0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 70
mode = sys.argv[3] if len(sys.argv) > 3 else "boxes"
TOL, MAXIT, T, REPS = 1e-5, 5000, 4, 50
rp, ci, v = gen.elasticity3d_csr(n)
N = len(rp) - 1
if mode == "boxes":
    part, P = gen.box_partition_nodes(n, (2, 4, 8))
    prob = pa.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
else:
    P = 64
    prob = pa.EcgProblem(rp, ci, v, P, None, scale=True, device=0, partitioner=True)
pa.lib.check(prob.L.preAlps_hip_prepare_operator(T), "prepare")
t0 = time.perf_counter()
prob.create_block_jacobi()
prob.sync()
print("elasticity %d^3, %s: %d parts, block-Jacobi create %.3f s, %d sparse-factored blocks"
      % (n, mode, P, time.perf_counter() - t0, prob.stat("bj_nd_blocks")), flush=True)
V = nearkernel.translations(N, 3)
b = np.random.default_rng(7).standard_normal(prob.m)
W = np.random.default_rng(8).standard_normal((prob.m, T))
dx, dy = prob.panel(T, T), prob.panel(T, T)
prob.to_device(dx, W, T)


def apply_seconds():
    L = prob.L
    for _ in range(5):
        pa.lib.check(L.preAlps_BlockJacobiApply(C.byref(dx), C.byref(dy)), "apply")
    s = C.c_double()
    pa.lib.check(L.preAlps_hip_timer_start(), "timer")
    for _ in range(REPS):
        pa.lib.check(L.preAlps_BlockJacobiApply(C.byref(dx), C.byref(dy)), "apply")
    pa.lib.check(L.preAlps_hip_timer_stop(C.byref(s)), "timer")
    return s.value / REPS


out = {"plain": [], "coarse": []}
for r in range(rounds):
    for way in (("plain", "coarse") if r % 2 == 0 else ("coarse", "plain")):
        setup = 0.0
        if way == "coarse":
            prob.set_coarse_space(V)
            setup = prob.stat("bj_coarse_setup_s")
        else:
            prob.clear_coarse_space()
        prob.sync()
        got = prob.solve(b, T, tol=TOL, max_iter=MAXIT)
        ap = apply_seconds()
        rec = dict(iters=got.iters, seconds=got.seconds, us_per_iter=1e6 * got.seconds / max(got.iters, 1),
                   apply_us=1e6 * ap, setup_s=setup, converged=bool(got.final_res <= TOL * got.normb))
        out[way].append(rec)
        print("round %d %-6s %5d iterations  %8.4f s  %7.1f us/iteration  apply %7.1f us  setup %.3f s  %s"
              % (r, way, rec["iters"], rec["seconds"], rec["us_per_iter"], rec["apply_us"], setup,
                 "" if rec["converged"] else "NOT CONVERGED"), flush=True)
prob.set_coarse_space(V)
summary = dict(n=n, mode=mode, parts=P, t=T, tol=TOL, rounds=rounds,
               coarse_dofs=prob.stat("bj_coarse_dofs"), aggregates=prob.stat("bj_coarse_aggregates"),
               chunks=prob.stat("bj_coarse_chunks"), coarse_bytes=prob.stat("bj_coarse_bytes"))
for way in out:
    for key in ("iters", "seconds", "us_per_iter", "apply_us", "setup_s"):
        summary["%s_%s_median" % (way, key)] = float(np.median([x[key] for x in out[way]]))
summary["coarse_stages_us"] = summary["coarse_apply_us_median"] - summary["plain_apply_us_median"]
print(json.dumps(summary))
prob.panel_free(dx)
prob.panel_free(dy)
prob.close()
