"""The matrices of tests/test_spmm_code_cpu.py and tests/test_gpu_spmm_code.py: Q1 elasticity, whose assembled values
repeat a few bit patterns, and variants that take the repetition away everywhere, in a quarter of the rows, or plant
patterns that compare equal or unordered as values but are different bits."""
import numpy as np

SPECIAL_NEGZEROS = 3
DENORMAL = np.array([0x0000000000000123], dtype=np.uint64).view(np.float64)[0]
NAN_A = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
NAN_B = np.array([0x7FF8000000000002], dtype=np.uint64).view(np.float64)[0]


def base(kind):
    """rowptr, colind, val, parts, partition vector."""
    from prealps_amd import gen
    if kind == "elasticity7":
        rp, ci, v = gen.elasticity3d_csr(7)
        n = len(rp) - 1
        cut = [(p * n) // 8 for p in range(9)]             # 8 contiguous parts: nodes are cut apart (test_spmm_pack_cpu.py)
        return rp, ci, v, 8, np.repeat(np.arange(8, dtype=np.int32), np.diff(cut))
    if kind == "elasticity12":
        nn = (12, 10, 10)
        rp, ci, v = gen.elasticity3d_csr(nn)
        part, P = gen.box_partition_nodes(nn, (2, 2, 2))
        return rp, ci, v, P, np.asarray(part, dtype=np.int32)
    raise KeyError(kind)


def distinct(v, seed=20261020):
    """every stored value that is not +0.0 replaced by a random one of its own (no two alike)"""
    out = v.copy()
    nz = np.flatnonzero(out.view(np.uint64) != 0)
    r = np.random.default_rng(seed).permutation(len(nz)).astype(np.float64)
    out[nz] = (1.0 + r / len(nz)) * np.where(out[nz] < 0, -1.0, 1.0)      # all different, all in [1, 2) in magnitude
    assert len(np.unique(out[nz].view(np.uint64))) == len(nz)
    return out


def mixed(rp, v, rows_lo, rows_hi, seed=7):
    """distinct random factors on the values of rows [rows_lo, rows_hi)"""
    out = v.copy()
    a, b = rp[rows_lo], rp[rows_hi]
    out[a:b] *= 1.0 + np.random.default_rng(seed).random(b - a)
    return out


def special(rp, ci, v):
    """a few -0.0 in places that held +0.0, a denormal and two NaNs of different payload in places that held values"""
    out = v.copy()
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    zeros = np.flatnonzero((out.view(np.uint64) == 0) & (rows != ci))
    out[zeros[:: len(zeros) // SPECIAL_NEGZEROS][:SPECIAL_NEGZEROS]] = -0.0
    vals = np.flatnonzero((out.view(np.uint64) != 0) & (rows != ci) & (out != 0))
    k = len(vals) // 4
    out[vals[k]] = DENORMAL
    out[vals[2 * k]] = NAN_A
    out[vals[3 * k]] = NAN_B
    return out
