"""The SpMM block-shape cases of test_spmm_blocks_cpu.py (the plan builder alone, no GPU) and test_gpu_spmm_blocks.py
(the kernels that consume those plans): matrices of gen.node_graph_csr at the smallest row counts at which a device
of 256 compute units is given blocks of two, three and four slices (block_rows() of spmm_plan.c: from 131 072,
196 608 and 262 144 rows), their partitions, the switch settings, and GEOMETRY -- what pa_spmm_plan_build cuts for
every (case, panel stride, switch setting) at cus = 256.  The CPU test holds the builder against GEOMETRY and GEOMETRY
against the conditions the cases exist for; the GPU test holds the statistics of the plan that ran against GEOMETRY.

Not a test module: nothing here is collected."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
CUS = 256
STRIDES = (2, 4, 8, 16)

# name -> (nodes, node_graph_csr keywords, parts, seed of random cuts or None for floor(r P / N))
CASES = {
    "base4": (87424, dict(), 683, None),                            # 262 272 rows, parts of 384 rows
    "far2": (87424, dict(far_every=2, nfar=2), 683, None),
    "far3": (87424, dict(far_every=1, nfar=3), 683, None),
    "three": (65600, dict(), 512, None),                            # 196 800 rows
    "two": (43712, dict(), 341, None),                              # 131 136 rows
    "ragged": (87424, dict(), 2600, 3),                             # base4's matrix, parts of 1 .. some hundred rows
}
GRAPH_STRIDE, GRAPH_SEED = 300, 1

# name -> (PREALPS_SPMM_STAGED, PREALPS_SPMM_RUNS); "default" leaves both unset (-1, 1)
SWITCHES = {"default": (-1, 1), "runs": (-1, 2), "staged": (1, 0), "window": (0, 1)}


def switch_env(switch):
    """The environment of a switch setting: name -> value, None = unset."""
    staged, runs = SWITCHES[switch]
    if switch == "default":
        return {"PREALPS_SPMM_STAGED": None, "PREALPS_SPMM_RUNS": None}
    return {"PREALPS_SPMM_STAGED": str(staged), "PREALPS_SPMM_RUNS": str(runs)}


def stride_of(t):
    """The panel stride of t columns: 2, 4, 8 or 16."""
    ts = 2
    while ts < t:
        ts <<= 1
    return ts


@functools.lru_cache(maxsize=2)
def _graph(nn, kw, excess):
    from prealps_amd import gen
    out = gen.node_graph_csr(nn, GRAPH_STRIDE, GRAPH_SEED, excess=excess, **dict(kw))
    for a in out:
        a.setflags(write=False)
    return out


def matrix(name, excess=1.0):
    """(rowptr, colind, val) of the case, read-only; the last two graphs stay cached."""
    nn, kw, _, _ = CASES[name]
    return _graph(nn, tuple(sorted(kw.items())), float(excess))


@functools.lru_cache(maxsize=None)
def partition(name):
    """(part vector, parts, rowpos): contiguous parts, so the library permutes nothing."""
    nn, _, P, cut_seed = CASES[name]
    N = 3 * nn
    if cut_seed is None:
        part = (np.arange(N, dtype=np.int64) * P // N).astype(np.int32)
    else:
        cuts = np.sort(np.random.default_rng(cut_seed).choice(np.arange(1, N), P - 1, replace=False))
        part = np.repeat(np.arange(P, dtype=np.int32), np.diff(np.concatenate([[0], cuts, [N]])))
    rowpos = np.zeros(P + 1, dtype=np.int32)
    rowpos[1:] = np.cumsum(np.bincount(part, minlength=P))
    part.setflags(write=False)
    rowpos.setflags(write=False)
    return part, P, rowpos


# ---- what spmm_plan.c allows ------------------------------------------------------------------------------------
def nominal_slices(rows, dflt_rows=256, cus=CUS):
    """block_rows() / 64 before the staging cap: slices of a full block."""
    r = dflt_rows
    while r > 64 and rows // r < 4 * cus:
        r -= 64
    return max(r, 64) // 64


def stage_cap(ts, runs):
    """The largest spmm_stage_rows plan_staged() accepts at stride ts (run plan: two zero rows included)."""
    if runs:
        if ts >= 16:
            ts //= 2
        return (32768 if ts <= 4 else 81920) // (80 if ts == 8 else ts * 8)
    return (32768 if ts <= 4 else 49152) // (ts * 8)


def stage_bytes(ts, runs, stage_rows):
    """Dynamic LDS of the launch (launch_spmm: rows of 8-column panels are 80 bytes apart)."""
    if runs and ts >= 16:
        ts //= 2
    return stage_rows * (80 if ts == 8 else ts * 8)


# ---- the plan builder through ctypes (spmm_plan.h) --------------------------------------------------------------
_pi, _pd = C.POINTER(C.c_int), C.POINTER(C.c_double)


class PlanIn(C.Structure):       # pa_spmm_plan_in_t
    _fields_ = [("m", C.c_int), ("halo", C.c_int), ("part0", C.c_int), ("part1", C.c_int), ("row_off", C.c_int),
                ("rowPos", _pi), ("rowPtr", _pi), ("lcol", _pi), ("val", _pd), ("ts", C.c_int), ("cus", C.c_int),
                ("want_staged", C.c_int), ("want_runs", C.c_int)]


class PlanArray(C.Structure):    # pa_plan_array_t
    _fields_ = [("p", C.c_void_p), ("elem", C.c_size_t), ("n", C.c_size_t), ("n_alloc", C.c_size_t)]


PL_SL_NROWS, PL_BLK_SLICE, PL_COUNT = 3, 7, 13      # (the enum of spmm_plan.h)


class HostPlan(C.Structure):     # pa_spmm_host_plan_t
    _fields_ = [("m", C.c_int), ("nslices", C.c_int), ("nblk", C.c_int), ("n_interior", C.c_int), ("win_cap", C.c_int),
                ("staged", C.c_int), ("runs", C.c_int), ("runs_cols", C.c_int), ("stage_cap", C.c_int),
                ("sell_entries", C.c_double), ("stream_bytes", C.c_double), ("oom_entries", C.c_size_t),
                ("a", PlanArray * PL_COUNT)]


def compile_plan_library(tmpdir):
    """spmm_plan.c alone as a shared object (no sanitizer: test_spmm_plan_cpu.py has the sanitised builds)."""
    gcc = shutil.which("gcc")
    if gcc is None:
        raise RuntimeError("gcc is needed to build prealps_amd/csrc/spmm_plan.c")
    so = os.path.join(str(tmpdir), "libspmm_plan.so")
    subprocess.check_call([gcc, "-O2", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(CSRC, "spmm_plan.c"), "-o", so])
    L = C.CDLL(so)
    L.pa_spmm_plan_build.argtypes = [C.POINTER(PlanIn), C.POINTER(HostPlan)]
    L.pa_spmm_plan_build.restype = C.c_int
    L.pa_spmm_plan_free.argtypes = [C.POINTER(HostPlan)]
    L.pa_spmm_plan_free.restype = None
    return L


def build_plan(L, csr, rowpos, ts, switch, cus=CUS):
    """pa_spmm_plan_build for one process that owns every row.  Returns the scalars the library reports as
    statistics and, from blk_slice and sl_nrows, the slices of every block and the rows of every slice."""
    rp, ci, v = (np.ascontiguousarray(a) for a in csr)
    rowpos = np.ascontiguousarray(rowpos, dtype=np.int32)
    staged, runs = SWITCHES[switch]
    pin = PlanIn(len(rp) - 1, 0, 0, len(rowpos) - 1, 0, rowpos.ctypes.data_as(_pi), rp.ctypes.data_as(_pi),
                 ci.ctypes.data_as(_pi), v.ctypes.data_as(_pd), ts, cus, staged, runs)
    pl = HostPlan()
    rc = L.pa_spmm_plan_build(C.byref(pin), C.byref(pl))
    try:
        assert rc == 0, "pa_spmm_plan_build failed (%d)" % rc
        for which, elem in ((PL_BLK_SLICE, 4), (PL_SL_NROWS, 4)):
            assert pl.a[which].p and pl.a[which].elem == elem
        assert pl.a[PL_BLK_SLICE].n == pl.nblk + 1 and pl.a[PL_SL_NROWS].n == pl.nslices
        blk_slice = np.ctypeslib.as_array(C.cast(pl.a[PL_BLK_SLICE].p, _pi), shape=(pl.nblk + 1,)).copy()
        sl_nrows = np.ctypeslib.as_array(C.cast(pl.a[PL_SL_NROWS].p, _pi), shape=(pl.nslices,)).copy()
        return dict(runs=pl.runs, staged=pl.staged, slices=pl.nslices, blocks=pl.nblk, stage_rows=pl.stage_cap,
                    win_cap=pl.win_cap, blk_slice=blk_slice, sl_nrows=sl_nrows)
    finally:
        L.pa_spmm_plan_free(C.byref(pl))


def geometry_of(plan):
    """A plan as GEOMETRY records it: (runs, staged, slices, blocks, stage_rows, blocks of 1, 2, 3 and 4 slices)."""
    per = np.diff(plan["blk_slice"])
    assert per.min() >= 1 and per.max() <= 4
    hist = np.bincount(per, minlength=5)[1:5]
    return (plan["runs"], plan["staged"], plan["slices"], plan["blocks"], plan["stage_rows"], tuple(int(x) for x in hist))


# ---- the recorded geometry ----------------------------------------------------------------------------------------
# (case, stride, switch) -> (spmm_runs, spmm_staged, spmm_slices, spmm_blocks, spmm_stage_rows,
#                            (blocks of 1, 2, 3, 4 slices)); cut with spmm_plan.c at cus = 256
GEOMETRY = {
    ("base4", 2, "default"): (1, 1, 4098, 1025, 971, (0, 1, 0, 1024)),
    ("base4", 2, "runs"): (1, 1, 4098, 1025, 971, (0, 1, 0, 1024)),
    ("base4", 2, "staged"): (0, 1, 4098, 1025, 969, (0, 1, 0, 1024)),
    ("base4", 2, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("base4", 4, "default"): (0, 1, 4098, 1025, 969, (0, 1, 0, 1024)),
    ("base4", 4, "runs"): (1, 1, 4098, 1025, 971, (0, 1, 0, 1024)),
    ("base4", 4, "staged"): (0, 1, 4098, 1025, 969, (0, 1, 0, 1024)),
    ("base4", 4, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("base4", 8, "default"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("base4", 8, "runs"): (1, 1, 4098, 1025, 971, (0, 1, 0, 1024)),
    ("base4", 8, "staged"): (0, 1, 4098, 1366, 735, (0, 0, 1366, 0)),
    ("base4", 8, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("base4", 16, "default"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("base4", 16, "runs"): (1, 1, 4098, 1025, 971, (0, 1, 0, 1024)),
    ("base4", 16, "staged"): (0, 1, 4098, 4084, 360, (4070, 14, 0, 0)),
    ("base4", 16, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far2", 2, "default"): (1, 1, 4098, 1025, 1385, (0, 1, 0, 1024)),
    ("far2", 2, "runs"): (1, 1, 4098, 1025, 1385, (0, 1, 0, 1024)),
    ("far2", 2, "staged"): (0, 1, 4098, 1025, 1383, (0, 1, 0, 1024)),
    ("far2", 2, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far2", 4, "default"): (0, 1, 4098, 2046, 1023, (0, 2043, 0, 3)),
    ("far2", 4, "runs"): (1, 1, 4098, 2046, 1022, (0, 2043, 0, 3)),
    ("far2", 4, "staged"): (0, 1, 4098, 2046, 1023, (0, 2043, 0, 3)),
    ("far2", 4, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far2", 8, "default"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far2", 8, "runs"): (1, 1, 4098, 2046, 1022, (0, 2043, 0, 3)),
    ("far2", 8, "staged"): (0, 1, 4098, 2047, 768, (0, 2043, 4, 0)),
    ("far2", 8, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far2", 16, "default"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far2", 16, "runs"): (1, 1, 4098, 2046, 1022, (0, 2043, 0, 3)),
    ("far2", 16, "staged"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far2", 16, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 2, "default"): (0, 1, 4098, 2045, 2043, (0, 2041, 0, 4)),
    ("far3", 2, "runs"): (1, 1, 4098, 2045, 2045, (0, 2041, 0, 4)),
    ("far3", 2, "staged"): (0, 1, 4098, 2045, 2043, (0, 2041, 0, 4)),
    ("far3", 2, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 4, "default"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 4, "runs"): (1, 1, 4098, 4094, 1022, (4090, 4, 0, 0)),
    ("far3", 4, "staged"): (0, 1, 4098, 4093, 1023, (4088, 5, 0, 0)),
    ("far3", 4, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 8, "default"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 8, "runs"): (1, 1, 4098, 4094, 1022, (4090, 4, 0, 0)),
    ("far3", 8, "staged"): (0, 1, 4098, 4098, 696, (4098, 0, 0, 0)),
    ("far3", 8, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 16, "default"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 16, "runs"): (1, 1, 4098, 4094, 1022, (4090, 4, 0, 0)),
    ("far3", 16, "staged"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("far3", 16, "window"): (0, 0, 4098, 1366, 0, (0, 683, 0, 683)),
    ("three", 2, "default"): (1, 1, 3264, 1088, 737, (0, 0, 1088, 0)),
    ("three", 2, "runs"): (1, 1, 3264, 1088, 737, (0, 0, 1088, 0)),
    ("three", 2, "staged"): (0, 1, 3264, 1088, 735, (0, 0, 1088, 0)),
    ("three", 2, "window"): (0, 0, 3264, 1216, 0, (192, 0, 1024, 0)),
    ("three", 4, "default"): (0, 1, 3264, 1088, 735, (0, 0, 1088, 0)),
    ("three", 4, "runs"): (1, 1, 3264, 1088, 737, (0, 0, 1088, 0)),
    ("three", 4, "staged"): (0, 1, 3264, 1088, 735, (0, 0, 1088, 0)),
    ("three", 4, "window"): (0, 0, 3264, 1216, 0, (192, 0, 1024, 0)),
    ("three", 8, "default"): (0, 0, 3264, 1216, 0, (192, 0, 1024, 0)),
    ("three", 8, "runs"): (1, 1, 3264, 1088, 737, (0, 0, 1088, 0)),
    ("three", 8, "staged"): (0, 1, 3264, 1088, 735, (0, 0, 1088, 0)),
    ("three", 8, "window"): (0, 0, 3264, 1216, 0, (192, 0, 1024, 0)),
    ("three", 16, "default"): (0, 0, 3264, 1216, 0, (192, 0, 1024, 0)),
    ("three", 16, "runs"): (1, 1, 3264, 1088, 737, (0, 0, 1088, 0)),
    ("three", 16, "staged"): (0, 1, 3264, 3058, 354, (2854, 202, 2, 0)),
    ("three", 16, "window"): (0, 0, 3264, 1216, 0, (192, 0, 1024, 0)),
    ("two", 2, "default"): (1, 1, 2238, 1119, 521, (0, 1119, 0, 0)),
    ("two", 2, "runs"): (1, 1, 2238, 1119, 521, (0, 1119, 0, 0)),
    ("two", 2, "staged"): (0, 1, 2238, 1119, 519, (0, 1119, 0, 0)),
    ("two", 2, "window"): (0, 0, 2238, 1215, 0, (192, 1023, 0, 0)),
    ("two", 4, "default"): (0, 1, 2238, 1119, 519, (0, 1119, 0, 0)),
    ("two", 4, "runs"): (1, 1, 2238, 1119, 521, (0, 1119, 0, 0)),
    ("two", 4, "staged"): (0, 1, 2238, 1119, 519, (0, 1119, 0, 0)),
    ("two", 4, "window"): (0, 0, 2238, 1215, 0, (192, 1023, 0, 0)),
    ("two", 8, "default"): (0, 0, 2238, 1215, 0, (192, 1023, 0, 0)),
    ("two", 8, "runs"): (1, 1, 2238, 1119, 521, (0, 1119, 0, 0)),
    ("two", 8, "staged"): (0, 1, 2238, 1119, 519, (0, 1119, 0, 0)),
    ("two", 8, "window"): (0, 0, 2238, 1215, 0, (192, 1023, 0, 0)),
    ("two", 16, "default"): (0, 0, 2238, 1215, 0, (192, 1023, 0, 0)),
    ("two", 16, "runs"): (1, 1, 2238, 1119, 521, (0, 1119, 0, 0)),
    ("two", 16, "staged"): (0, 1, 2238, 2034, 354, (1830, 204, 0, 0)),
    ("two", 16, "window"): (0, 0, 2238, 1215, 0, (192, 1023, 0, 0)),
    ("ragged", 2, "default"): (1, 1, 5511, 1378, 971, (0, 0, 1, 1377)),
    ("ragged", 2, "runs"): (1, 1, 5511, 1378, 971, (0, 0, 1, 1377)),
    ("ragged", 2, "staged"): (0, 1, 5511, 1378, 969, (0, 0, 1, 1377)),
    ("ragged", 2, "window"): (0, 0, 5511, 2822, 0, (1328, 711, 371, 412)),
    ("ragged", 4, "default"): (0, 1, 5511, 1378, 969, (0, 0, 1, 1377)),
    ("ragged", 4, "runs"): (1, 1, 5511, 1378, 971, (0, 0, 1, 1377)),
    ("ragged", 4, "staged"): (0, 1, 5511, 1378, 969, (0, 0, 1, 1377)),
    ("ragged", 4, "window"): (0, 0, 5511, 2822, 0, (1328, 711, 371, 412)),
    ("ragged", 8, "default"): (0, 0, 5511, 2822, 0, (1328, 711, 371, 412)),
    ("ragged", 8, "runs"): (1, 1, 5511, 1378, 971, (0, 0, 1, 1377)),
    ("ragged", 8, "staged"): (0, 1, 5511, 1837, 735, (0, 0, 1837, 0)),
    ("ragged", 8, "window"): (0, 0, 5511, 2822, 0, (1328, 711, 371, 412)),
    ("ragged", 16, "default"): (0, 0, 5511, 2822, 0, (1328, 711, 371, 412)),
    ("ragged", 16, "runs"): (1, 1, 5511, 1378, 971, (0, 0, 1, 1377)),
    ("ragged", 16, "staged"): (0, 1, 5511, 3714, 384, (2233, 1165, 316, 0)),
    ("ragged", 16, "window"): (0, 0, 5511, 2822, 0, (1328, 711, 371, 412)),
}

# the switch settings every case is run under on the GPU (one operator each)
GPU_SETTINGS = [(case, switch) for case in CASES
                for switch in ("default", "runs", "staged") + (("window",) if case in ("base4", "ragged") else ())]


def expected(case, t, switch):
    """GEOMETRY's record as the statistics the library reports after a product of t columns."""
    runs, staged, slices, blocks, stage_rows, hist = GEOMETRY[(case, stride_of(t), switch)]
    return dict(spmm_runs=runs, spmm_staged=staged, spmm_slices=slices, spmm_blocks=blocks, spmm_stage_rows=stage_rows)
