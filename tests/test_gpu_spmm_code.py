"""The packed run plan's values as 2-byte codes into per-block tables in LDS (PREALPS_SPMM_CODE, spmm_code.h): a
table lookup returns the 64 bits the packed array holds and every FMA runs in the same order, so every product, residual
history and solution has the bits of the plan without codes -- with every block coded, with coded and raw blocks in one
plan, and with -0.0, a denormal and NaNs of different payload among the values.  An update of the values forms the codes
anew or drops them; fp32 storage keeps no codes; the statistics are those of the host unit (tests/c/spmm_code_dump.c)."""
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

import spmm_code_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")

_SWITCHES = ("PREALPS_SPMM_STAGED", "PREALPS_SPMM_RUNS", "PREALPS_SPMM_PACK", "PREALPS_SPMM_GRAM", "PREALPS_SPMM_CODE",
             "PREALPS_SPMM_PRECISION")
_STATS = ("spmm_coded", "spmm_coded_blocks", "spmm_code_table_entries", "spmm_coded_stream_bytes", "spmm_recodes",
          "spmm_packed", "spmm_runs", "spmm_blocks", "spmm_packed_stream_bytes", "spmm_precision_stream_bytes",
          "spmm_stream_bytes", "spmm_precision")


def _env(monkeypatch, **env):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _matrix(kind):
    """rowptr, colind, val, parts, partition vector, scale."""
    rp, ci, v, P, part = K.base("elasticity12")
    n = len(rp) - 1
    if kind == "plain":
        return rp, ci, v, P, part, True
    # On a whole GPU a problem this small is cut into blocks of one slice.  Boxes of 2 x 2 x 2 nodes are slices of 24
    # rows, whose tables fit whatever the values; four contiguous parts are slices of 64 rows that reach some 500
    # external rows: 20 KiB of staging, so that the table of a block of rows without repetition (64 rows of ~50
    # values: 26 KiB) does not fit the 32 KiB and the block stays raw.
    four = np.repeat(np.arange(4, dtype=np.int32), n // 4)
    if kind == "distinct":
        return rp, ci, K.distinct(v), 4, four, True
    if kind == "mixed":
        # the factors on the first quarter of the rows; unscaled, so that the other rows keep their few patterns
        return rp, ci, K.mixed(rp, v, 0, n // 4), 4, four, False
    if kind == "special":
        return rp, ci, K.special(rp, ci, v), P, part, False      # (unscaled: a NaN in a row would take the scaling vector)
    raise KeyError(kind)


def _problem(mat, **kw):
    import prealps_amd
    rp, ci, v, P, part, scale = mat
    return prealps_amd.EcgProblem(rp, ci, v, P, part, scale=scale, device=0, **kw)


def _products(monkeypatch, mat, code, ts=(1, 2, 4), seed=5):
    """{t: A X} through a fresh operator with PREALPS_SPMM_CODE = code (None: unset), and per t its statistics."""
    _env(monkeypatch, **({} if code is None else {"PREALPS_SPMM_CODE": code}))
    prob = _problem(mat)
    out, stats = {}, {}
    try:
        for t in ts:
            X = np.random.default_rng(seed + t).standard_normal((prob.m, t))
            out[t] = prob.block_operator(X, t)
            stats[t] = {k: prob.stat(k) for k in _STATS}
    finally:
        prob.close()
    return out, stats


@pytest.mark.parametrize("kind", ["plain", "mixed", "special", "distinct"])
def test_coded_products_have_the_bits_of_the_plan_without_codes(kind, monkeypatch):
    mat = _matrix(kind)
    Y1, s1 = _products(monkeypatch, mat, 1)
    Y0, s0 = _products(monkeypatch, mat, 0)
    for t in (1, 2, 4):
        print("%s t=%d: %d of %d blocks coded, %d table entries, stream %.0f -> %.0f bytes" % (
            kind, t, s1[t]["spmm_coded_blocks"], s1[t]["spmm_blocks"], s1[t]["spmm_code_table_entries"],
            s1[t]["spmm_packed_stream_bytes"], s1[t]["spmm_coded_stream_bytes"]))
        assert s0[t]["spmm_coded"] == 0 and s0[t]["spmm_coded_blocks"] == 0 and s0[t]["spmm_coded_stream_bytes"] == 0
        assert s0[t]["spmm_packed"] == 1 and s1[t]["spmm_packed"] == 1 and s1[t]["spmm_runs"] == 1
        # (t = 1 runs at panel stride 2: the 2-column kernel; forced, every block that fits is coded)
        assert s1[t]["spmm_coded"] == 1, (kind, t)
        assert 0 < s1[t]["spmm_coded_blocks"] <= s1[t]["spmm_blocks"]
        assert s1[t]["spmm_coded_stream_bytes"] > 0
        # (spmm_precision_stream_bytes keeps pricing the storage precision alone: test_gpu_spmm_precision.py)
        assert s1[t]["spmm_precision_stream_bytes"] == s1[t]["spmm_packed_stream_bytes"]
        assert s1[t]["spmm_packed_stream_bytes"] == s0[t]["spmm_packed_stream_bytes"]
        assert _same_bits(Y1[t], Y0[t]), (kind, t)
        assert np.any(Y0[t] != 0.0)
    if kind == "plain":
        assert s1[4]["spmm_coded_blocks"] == s1[4]["spmm_blocks"]
        assert s1[4]["spmm_coded_stream_bytes"] < 0.6 * s1[4]["spmm_packed_stream_bytes"]
    if kind in ("mixed", "distinct"):                               # coded and raw blocks in one plan
        assert s1[4]["spmm_coded_blocks"] < s1[4]["spmm_blocks"]
    if kind == "special":
        assert np.isnan(Y0[4]).any() and np.isfinite(Y0[4]).any()


def test_the_default_codes_where_it_takes_a_tenth_off_the_stream(monkeypatch):
    Yd, sd = _products(monkeypatch, _matrix("plain"), None, ts=(4,))
    assert sd[4]["spmm_coded"] == 1 and sd[4]["spmm_coded_stream_bytes"] < 0.9 * sd[4]["spmm_packed_stream_bytes"]
    Ym, sm = _products(monkeypatch, _matrix("mixed"), None, ts=(4,))
    assert sm[4]["spmm_coded"] == 1 and 0 < sm[4]["spmm_coded_blocks"] < sm[4]["spmm_blocks"]
    Y0, _ = _products(monkeypatch, _matrix("mixed"), 0, ts=(4,))
    assert _same_bits(Ym[4], Y0[4])
    Yn, sn = _products(monkeypatch, _matrix("distinct"), None, ts=(4,))
    assert sn[4]["spmm_coded"] == 0 and sn[4]["spmm_coded_blocks"] == 0 and sn[4]["spmm_packed"] == 1
    assert sn[4]["spmm_precision_stream_bytes"] == sn[4]["spmm_packed_stream_bytes"]


def test_solver_history_and_solution_have_the_same_bits(monkeypatch):
    """12 iterations of Orthodir at t = 4 through the library's loop: the Gram kernel on the coded plan (all blocks coded,
    and coded beside raw blocks)."""
    import prealps_amd as pa
    for kind in ("plain", "mixed"):
        got = {}
        for code in (1, 0):
            _env(monkeypatch, PREALPS_SPMM_CODE=code)
            prob = _problem(_matrix(kind))
            try:
                rhs = prob.reference_rhs()
                before = prob.stat("spmm_gram_launches")
                r = prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, tol=1e-30, max_iter=12)
                got[code] = (r, prob.stat("spmm_gram_launches") - before, prob.stat("spmm_coded"))
            finally:
                prob.close()
        (r1, g1, c1), (r0, g0, c0) = got[1], got[0]
        assert c1 == 1 and c0 == 0 and r1.iters == r0.iters == 12 and g1 == g0 > 0
        assert np.isfinite(r1.res).all() and _same_bits(r1.res, r0.res) and _same_bits(r1.x, r0.x), kind


def _scaled(rp, ci, v):                   # S A S (test_gpu_update_values.py): every value changes, zeros stay zero
    N = len(rp) - 1
    s = 1.0 + 0.3 * (2.0 * np.random.default_rng(20261018).random(N) - 1.0)
    rows = np.repeat(np.arange(N), np.diff(rp))
    return s[rows] * v * s[ci]


def test_update_forms_the_codes_anew_or_drops_them(monkeypatch):
    rp, ci, v, P, part, _ = _matrix("plain")
    # the same pattern with other repeated values; then a dropped zero and its mirror image become nonzero; then
    # values without repetition
    v2 = 1.5 * v
    v3 = v2.copy()
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    zero = np.flatnonzero((v2.view(np.uint64) == 0) & (rows != ci))
    k = zero[len(zero) // 2]
    mirror = np.flatnonzero((rows == ci[k]) & (ci == rows[k]))[0]
    v3[k] = v3[mirror] = -1e-3
    v4 = K.distinct(v3)                                                # (the same places: written through the pack)
    X = np.random.default_rng(4).standard_normal((len(rp) - 1, 4))
    _env(monkeypatch)                                                  # the default rule
    prob = _problem((rp, ci, v, P, part, True))
    try:
        prob.block_operator(X, 4)
        assert prob.stat("spmm_coded") == 1 and prob.stat("spmm_recodes") == 0
        at = prob.stat("spmm_val_address")
        prob.update_values(v2)
        assert prob.stat("spmm_val_address") == at and prob.stat("spmm_repacks") == 0      # written through the pack ...
        assert prob.stat("spmm_coded") == 1 and prob.stat("spmm_recodes") == 1             # ... and coded anew
        Y2 = prob.block_operator(X, 4)
        prob.update_values(v3)
        assert prob.stat("spmm_repacks") == 1 and prob.stat("spmm_coded") == 1 and prob.stat("spmm_recodes") == 2
        Y3 = prob.block_operator(X, 4)
        prob.update_values(v4)
        assert prob.stat("spmm_repacks") == 1 and prob.stat("spmm_recodes") == 3
        assert prob.stat("spmm_coded") == 0 and prob.stat("spmm_coded_blocks") == 0 and prob.stat("spmm_packed") == 1
        assert prob.stat("spmm_precision_stream_bytes") == prob.stat("spmm_packed_stream_bytes")
        Y4 = prob.block_operator(X, 4)
    finally:
        prob.close()
    for vals, Y in ((v2, Y2), (v3, Y3), (v4, Y4)):
        _env(monkeypatch, PREALPS_SPMM_CODE=0)
        f = _problem((rp, ci, vals, P, part, True))
        try:
            fresh = f.block_operator(X, 4)
        finally:
            f.close()
        assert _same_bits(Y, fresh)
    assert not np.array_equal(Y3, Y2)


def test_single_precision_keeps_no_codes(monkeypatch):
    mat = _matrix("plain")
    X = np.random.default_rng(8).standard_normal((len(mat[0]) - 1, 4))
    got = {}
    for code in (1, 0):
        _env(monkeypatch, PREALPS_SPMM_CODE=code)
        prob = _problem(mat)
        try:
            Y64 = prob.block_operator(X, 4)
            assert prob.stat("spmm_coded") == code
            prob.set_operator_precision("single")
            assert prob.stat("spmm_precision") == 32 and prob.stat("spmm_coded") == 0 and prob.stat("spmm_coded_blocks") == 0
            Y32 = prob.block_operator(X, 4)
            prob.set_operator_precision("double")
            assert prob.stat("spmm_precision") == 64 and prob.stat("spmm_coded") == code
            got[code] = (Y64, Y32, prob.block_operator(X, 4))
        finally:
            prob.close()
    assert _same_bits(got[1][0], got[0][0]) and _same_bits(got[1][1], got[0][1]) and _same_bits(got[1][2], got[0][0])
    assert not np.array_equal(got[0][1], got[0][0])
    _env(monkeypatch, PREALPS_SPMM_CODE=1, PREALPS_SPMM_PRECISION="single")      # 32 in force at the build
    prob = _problem(mat)
    try:
        Y = prob.block_operator(X, 4)
        assert prob.stat("spmm_precision") == 32 and prob.stat("spmm_coded") == 0
    finally:
        prob.close()
    assert _same_bits(Y, got[0][1])


def test_statistics_agree_with_the_host_unit(monkeypatch, tmp_path):
    """The operator's own panel through tests/c/spmm_code_dump.c, cut for the device's compute units."""
    import torch
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/spmm_code_dump.c")
    exe = str(tmp_path / "spmm_code_dump")
    subprocess.check_call([gcc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "spmm_code_dump.c")] +
                          [os.path.join(CSRC, u + ".c") for u in ("spmm_plan", "spmm_pack", "spmm_code")] + ["-o", exe])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for kind in ("plain", "mixed"):
        mat = _matrix(kind)
        _env(monkeypatch, PREALPS_SPMM_CODE=1)
        prob = _problem(mat)
        try:
            prob.block_operator(np.ones((prob.m, 4)), 4)
            s = {k: prob.stat(k) for k in _STATS}
            rp, ci, v = prob.local_csr()
        finally:
            prob.close()
        sizes = np.bincount(mat[4], minlength=mat[3])
        path = str(tmp_path / kind)
        with open(path, "wb") as f:
            np.array([len(rp) - 1, mat[3], len(v)], dtype=np.int32).tofile(f)
            np.concatenate(([0], np.cumsum(sizes))).astype(np.int32).tofile(f)
            rp.astype(np.int32).tofile(f)
            ci.astype(np.int32).tofile(f)
            v.astype(np.float64).tofile(f)
        run = subprocess.run([exe, "4", "32768", path, path + ".bin", str(cus)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.startswith(kind + ": ok "), run.stdout + run.stderr
        r = {k: float(x) for k, x in (kv.split("=") for kv in run.stdout.split()[2:])}
        assert r["nblk"] == s["spmm_blocks"] and r["stream_bytes"] == s["spmm_stream_bytes"], kind
        assert (r["ncoded"], r["ntab"]) == (s["spmm_coded_blocks"], s["spmm_code_table_entries"]), kind
        assert s["spmm_packed_stream_bytes"] == r["stream_bytes"] - r["unpacked_bytes"] + r["packed_bytes"]
        assert s["spmm_coded_stream_bytes"] == r["stream_bytes"] - r["unpacked_bytes"] + r["coded_bytes"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, code, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["LOCAL_RANK"] = "0"
        for k in _SWITCHES:
            os.environ.pop(k, None)
        if code is not None:
            os.environ["PREALPS_SPMM_CODE"] = str(code)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import prealps_amd as pa
        rp, ci, v, P, part, scale = _matrix("plain")
        prob = pa.EcgProblem(rp, ci, v, P, part, scale=scale, device=0, distributed=True)
        rhs = prob.reference_rhs()
        r = prob.solve(rhs, 4, ortho_alg=pa.ORTHODIR, tol=1e-30, max_iter=12)
        out = (rank, "ok", r.res.copy(), r.x.copy(), prob.stat("spmm_coded"), prob.stat("halo_rows"))
        prob.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put(out)
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: %s\n%s" % (e, traceback.format_exc())))


def test_two_ranks_one_gpu_default_rule_matches_no_codes():
    import torch.multiprocessing as mp
    got = {}
    for code in (None, 0):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, code, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=240) for _ in procs]
        for p in procs:
            p.join(timeout=60)
        for r in res:
            assert r[1] == "ok", r
        got[code] = {r[0]: r for r in res}
    for rank in (0, 1):
        d, n = got[None][rank], got[0][rank]
        assert d[4] == 1 and n[4] == 0 and d[5] > 0
        assert len(d[2]) > 0 and np.isfinite(d[2]).all()
        assert _same_bits(d[2], n[2]) and _same_bits(d[3], n[3])
