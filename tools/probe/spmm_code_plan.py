#!/usr/bin/env python3
"""The headline problem's SpMM plan with and without 2-byte codes (PREALPS_SPMM_CODE=0 / unset, twice each): the
statistics of the coded plan and the seconds the plan build takes (cut, pack, code, upload).  Run from the repo root on
a GPU:  python tools/probe/spmm_code_plan.py"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import prealps_amd
from prealps_amd import gen

KEYS = ("spmm_coded", "spmm_blocks", "spmm_coded_blocks", "spmm_code_table_entries", "spmm_stream_bytes",
        "spmm_packed_stream_bytes", "spmm_coded_stream_bytes", "spmm_precision_stream_bytes", "spmm_code_lds_bytes",
        "spmm_stage_rows", "setup_plan_s")

rp, ci, v = gen.elasticity3d_csr(70)
part, P = gen.box_partition_nodes(70, (2, 4, 8))
for code in ("0", None, "0", None):
    if code is None:
        os.environ.pop("PREALPS_SPMM_CODE", None)
    else:
        os.environ["PREALPS_SPMM_CODE"] = code
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    t0 = time.perf_counter()
    prealps_amd.lib.check(prob.L.preAlps_hip_prepare_operator(4), "preAlps_hip_prepare_operator")
    dt = time.perf_counter() - t0
    print("PREALPS_SPMM_CODE=%s prepare %.3f s " % (code, dt) + " ".join("%s=%.10g" % (k, prob.stat(k)) for k in KEYS), flush=True)
    prob.close()
