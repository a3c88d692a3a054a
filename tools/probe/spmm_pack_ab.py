#!/usr/bin/env python3
"""One process, the headline problem, PREALPS_SPMM_PACK = 0 / 1 in alternating windows: the switch is read when the
SpMM plan is cut, so every window first takes a product at another panel stride (the plan is cut anew on the way back)
and then times an 800-iteration solve.  usage: spmm_pack_ab.py [rounds]   (R4_AB_T: columns, R4_AB_N: nodes per side)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import prealps_amd
from prealps_amd import gen
t = int(os.environ.get("R4_AB_T", "4"))
n = int(os.environ.get("R4_AB_N", "70"))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
rp, ci, v = gen.elasticity3d_csr(n); part, P = gen.box_partition_nodes(n, (2, 4, 8))
prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
rhs = prob.reference_rhs()
prob.solve(rhs, t, tol=1e-30, max_iter=50)
X8 = np.zeros((prob.m, 8))
for rnd in range(rounds):
    for pack in ("0", "1"):
        os.environ["PREALPS_SPMM_PACK"] = pack
        prob.block_operator(X8, 8)
        prob.solve(rhs, t, tol=1e-30, max_iter=20)
        r = prob.solve(rhs, t, tol=1e-30, max_iter=800)
        print("round %d PREALPS_SPMM_PACK=%s packed=%d stream %.1f MB (unpacked %.1f MB): %d iterations, %.1f us per iteration"
              % (rnd, pack, prob.stat("spmm_packed"), prob.stat("spmm_packed_stream_bytes") / 1e6,
                 prob.stat("spmm_stream_bytes") / 1e6, r.iters, 1e6 * r.seconds / r.iters), flush=True)
prob.close()
