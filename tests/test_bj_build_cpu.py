"""The host unit of the block-Jacobi create (prealps_amd/csrc/bj_build.c): factor order, band assembly, host band
Cholesky, the sweep records of a host-factored block and the layout table.  tests/c/bj_build_check.c, a stand-alone
program built with AddressSanitizer + UBSan together with bj_build.c alone, runs the unit on the cases written here
and dumps every array; the comparisons are made here, against numpy restatements of the documented rules.

Panels: Poisson 12^3 in 8 contiguous parts; the 3-dof node grid 8^3 in boxes of 4^3 nodes (the pattern and the
off-diagonal values of tests/c/bj_band_map_check.c, with a dominant diagonal so that the blocks factor);
gen.band_blocks_csr with the BLOCKS of test_band_blocks_cpu.py, plain and shuffled; blocks 2..5 of the Poisson panel
as a shard (row_off > 0, halo columns present); and three blocks of 257 / 257 / 20 rows for the slab layout.
tests/golden/bj_build_orders.json pins the factor orders and bandwidths of all of them to those of the create before
the unit was split out of block_jacobi.c (sha256 of the int32 order of every block)."""
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from prealps_amd import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bj_build_orders.json")

BLOCKS = [(1, 0), (2, 1), (3, 5), (5, 4), (16, 15), (17, 5), (64, 33), (65, 64), (130, 112), (192, 0), (256, 80)]
SLABS = [(257, 9), (257, 120), (20, 3)]
WIDE_FROM = 96                      # the slab layout of the block cases: bands above it in window-slot order
FACTOR_WMAX, MAX_R, G4_MAX_BAND, G4_MAX_ROWS = 96, 8, 112, 256      # the kernels' constants, as block_jacobi.c passes them
OK, NOMEM, NOT_SPD, BANDWIDTH = 0, -1, -2, -3


# ---- the panels ------------------------------------------------------------------------------------------------
def _panel(rp, ci, v, rowpos, p0, p1):
    """rows of the parts [p0, p1) of a matrix whose rows are grouped by part: local rows, global column ids"""
    lo, hi = int(rowpos[p0]), int(rowpos[p1])
    return dict(grow=np.asarray(rowpos[p0:p1 + 1], np.int32), rp=(rp[lo:hi + 1] - rp[lo]).astype(np.int32),
                ci=np.ascontiguousarray(ci[rp[lo]:rp[hi]], np.int32), v=np.ascontiguousarray(v[rp[lo]:rp[hi]], np.float64),
                row_off=lo, m=hi - lo, np=p1 - p0)


def _nodes8():
    g, dof = 8, 3
    node = np.arange(g ** 3)
    x, y, z = node % g, (node // g) % g, node // (g * g)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = (x + dx >= 0) & (x + dx < g) & (y + dy >= 0) & (y + dy < g) & (z + dz >= 0) & (z + dz < g)
                a, b = node[ok], ((z + dz) * g + (y + dy))[ok] * g + (x + dx)[ok]
                for d in range(dof):
                    for e in range(dof):
                        rows.append(a * dof + d)
                        cols.append(b * dof + e)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    vals = -(1.0 + ((lo * 31 + hi * 17) % 7) / 8.0)
    vals[rows == cols] = 0.0
    A = sp.csr_matrix((vals, (rows, cols)), shape=(g ** 3 * dof,) * 2)
    A = A + sp.diags(1.0 + np.asarray(abs(A).sum(axis=1)).ravel())           # dominant diagonal: SPD
    part = ((z // 4) * 4 + (y // 4) * 2 + x // 4).repeat(dof)
    perm = np.argsort(part, kind="stable")
    B = sp.csr_matrix(A[perm][:, perm])
    B.sort_indices()
    rowpos = np.concatenate([[0], np.cumsum(np.bincount(part, minlength=8))])
    return _panel(B.indptr, B.indices, B.data, rowpos, 0, 8)


def _band_panel(blocks, seed, **kw):
    rp, ci, v, part, P = gen.band_blocks_csr(blocks, seed=seed, **kw)
    rowpos = np.concatenate([[0], np.cumsum([b for b, _ in blocks])])
    return _panel(rp, ci, v, rowpos, 0, P)


def panels():
    rp, ci, v = gen.poisson3d_csr(12)
    rowpos = np.arange(9) * (12 ** 3 // 8)
    return {"poisson12": _panel(rp, ci, v, rowpos, 0, 8), "nodes8": _nodes8(),
            "band": _band_panel(BLOCKS, 1), "band_shuffled": _band_panel(BLOCKS, 1, shuffle=True),
            "poisson12_shard": _panel(rp, ci, v, rowpos, 2, 6), "slabs": _band_panel(SLABS, 3)}


def block_case(P, dev_factor, dev_wmax, threads=1, nd_mode=0, nd_rows=2048, wide_from=WIDE_FROM):
    head = [1, P["np"], P["m"], len(P["ci"]), P["row_off"], nd_mode, nd_rows, dev_factor, dev_wmax, threads, wide_from]
    return np.asarray(head, np.int32).tobytes() + P["grow"].tobytes() + P["rp"].tobytes() + P["ci"].tobytes() + P["v"].tobytes()


def layout_case(nrows, bw, is_nd, dev_factor, wide_from, want_g4, want_pairs):
    head = [2, len(nrows), FACTOR_WMAX, MAX_R, G4_MAX_BAND, G4_MAX_ROWS, dev_factor, wide_from, want_g4, want_pairs]
    return b"".join(np.asarray(a, np.int32).tobytes() for a in (head, nrows, bw, is_nd))


def cholesky_case(band):
    b, ld = band.shape
    return np.asarray([3, b, ld - 1], np.int32).tobytes() + np.ascontiguousarray(band, np.float64).tobytes()


def read_arrays(path):
    """{case: {field: array}} of the program's output"""
    out, kinds = {}, {"i": np.int32, "q": np.int64, "d": np.float64, "c": np.uint8}
    with open(path, "rb") as f:
        data = f.read()
    at = 0
    while at < len(data):
        name = data[at:at + 32].split(b"\0", 1)[0].decode()
        kind, (count,) = chr(data[at + 32]), struct.unpack_from("<q", data, at + 33)
        at += 41
        arr = np.frombuffer(data, kinds[kind], count, at)
        at += arr.nbytes
        case, field = name.split(".", 1)
        out.setdefault(int(case), {})[field] = arr
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/bj_build_check.c")
    tmp = tmp_path_factory.mktemp("bj_build")
    exe, unit = str(tmp / "bj_build_check"), str(tmp / "bj_build.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "bj_build.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "bj_build_check.c"), unit, "-o", exe, "-lm"])
    return exe


def run_cases(exe, tmp, cases):
    src, dst = os.path.join(str(tmp), "cases.bin"), os.path.join(str(tmp), "arrays.bin")
    with open(src, "wb") as f:
        f.write(b"".join(cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    out = read_arrays(dst)
    assert sorted(out) == list(range(len(cases)))
    return [out[c] for c in range(len(cases))]


# ---- the block cases: run once, shared -----------------------------------------------------------------------
CONFIGS = [("dev96", dict(dev_factor=1, dev_wmax=96, threads=3)), ("dev8", dict(dev_factor=1, dev_wmax=8)),
           ("host", dict(dev_factor=0, dev_wmax=96, threads=3))]


@pytest.fixture(scope="module")
def built(exe, tmp_path_factory):
    """{(panel, config): (panel, the program's arrays)}"""
    Ps = panels()
    keys = [(name, cfg) for name in Ps for cfg, _ in CONFIGS]
    res = run_cases(exe, tmp_path_factory.mktemp("blocks"), [block_case(Ps[name], **dict(CONFIGS)[cfg]) for name, cfg in keys])
    assert all(int(r["rc"][0]) == OK for r in res)
    return {k: (Ps[k[0]], r) for k, r in zip(keys, res)}


def _blocks(P, r):
    """per block: q, r0, b, g0, order, bw"""
    for q in range(P["np"]):
        r0, b = int(r["row0"][q]), int(r["nrows"][q])
        yield q, r0, b, int(P["grow"][q]), r["map_f"][r0:r0 + b], int(r["bw"][q])


def _dense_block(P, r0, b, g0):
    """the diagonal block in the given order"""
    rp, ci, v = P["rp"], P["ci"], P["v"]
    rows = np.repeat(np.arange(b), np.diff(rp[r0:r0 + b + 1]))
    cols, vals = ci[rp[r0]:rp[r0 + b]] - g0, v[rp[r0]:rp[r0 + b]]
    inb = (cols >= 0) & (cols < b)
    D = np.zeros((b, b))
    D[rows[inb], cols[inb]] = vals[inb]
    return D


def _bandwidth(D):
    i, j = np.nonzero(D)
    off = i != j
    return int(np.abs(i - j)[off].max()) if off.any() else 0


def _band_of(Dp, w):
    """band[i, d] = Dp[i, i - d], zero where i - d < 0"""
    b = Dp.shape[0]
    band = np.zeros((b, w + 1))
    for d in range(min(w, b - 1) + 1):
        band[d:, d] = Dp[np.arange(d, b), np.arange(0, b - d)]
    return band


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_orders_are_permutations_with_the_reported_bandwidth(built):
    natural, rcm = {}, {}
    for (name, cfg), (P, r) in built.items():
        assert np.array_equal(r["row0"], P["grow"][:-1] - P["row_off"]) and np.array_equal(r["nrows"], np.diff(P["grow"]))
        assert not r["is_nd"].any()
        for q, r0, b, g0, order, w in _blocks(P, r):
            assert np.array_equal(np.sort(order), np.arange(b)), (name, cfg, q)
            assert np.array_equal(r["map_b"][r0:r0 + b], order[::-1])              # the backward sweep visits the reverse
            D = _dense_block(P, r0, b, g0)
            assert w == _bandwidth(D[np.ix_(order, order)]), (name, cfg, q)
            wnat = _bandwidth(D)
            assert w <= wnat
            ident = np.array_equal(order, np.arange(b))
            assert ident or w < wnat                                                # the given order wins a tie
            natural[name] = natural.get(name, 0) + (ident and b > 2)
            rcm[name] = rcm.get(name, 0) + (not ident)
    assert natural["band"] > 0 and rcm["band"] == 0            # a full band: no order is narrower than the given one
    assert rcm["band_shuffled"] > 0                            # reverse Cuthill-McKee's order, strictly narrower
    assert rcm["poisson12"] > 0 and rcm["poisson12_shard"] > 0


def test_orders_are_those_of_the_create_before_the_split(built):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted({name for name, _ in built})
    for (name, cfg), (P, r) in built.items():
        assert [int(w) for w in r["bw"]] == golden[name]["bw"], (name, cfg)
        got = [hashlib.sha256(np.ascontiguousarray(o, "<i4").tobytes()).hexdigest() for _, _, _, _, o, _ in _blocks(P, r)]
        assert got == golden[name]["order_sha256"], (name, cfg)


def test_a_shard_orders_its_blocks_as_the_whole_panel_does(built):
    whole, shard = built[("poisson12", "dev96")][1], built[("poisson12_shard", "dev96")][1]
    assert np.array_equal(shard["bw"], whole["bw"][2:6])
    assert np.array_equal(shard["map_f"], whole["map_f"][2 * 216:6 * 216])


def test_bands_are_the_permuted_diagonal_blocks(built):
    forms = set()
    for (name, cfg), (P, r) in built.items():
        dev_factor, dev_wmax = cfg != "host", 8 if cfg == "dev8" else 96
        if not dev_factor:
            continue                                     # (the host path holds the factor: test_host_cholesky_...)
        for q, r0, b, g0, order, w in _blocks(P, r):
            Dp = _dense_block(P, r0, b, g0)[np.ix_(order, order)]
            ref = _band_of(Dp, w)
            if w <= dev_wmax:                            # row-major band
                assert "coo_off%d" % q not in r
                assert _same_bits(r["band%d" % q].reshape(b, w + 1), ref), (name, cfg, q)
                forms.add((name, "rows"))
            else:                                        # entry list into the diagonal-major band
                assert "band%d" % q not in r
                off, val = r["coo_off%d" % q], r["coo_val%d" % q]
                assert len(np.unique(off)) == len(off) and off.min() >= 0 and off.max() < (w + 1) * b
                got = np.zeros((w + 1) * b)
                got[off] = val
                assert _same_bits(got.reshape(w + 1, b).T, ref), (name, cfg, q)
                assert len(off) == np.count_nonzero(np.tril(Dp))     # only the entries travel (none of them is zero)
                forms.add((name, "entries"))
    for name in ("poisson12", "nodes8", "band", "band_shuffled", "poisson12_shard"):
        assert (name, "rows") in forms and (name, "entries") in forms


def _dense_factor(band):
    b, ld = band.shape
    L = np.zeros((b, b))
    for d in range(min(ld, b)):
        L[np.arange(d, b), np.arange(0, b - d)] = band[d:, d]
    return L


def test_host_cholesky_meets_the_componentwise_bound(built):
    """|A - L L^T| <= (w + 3) u |L| |L^T| with u = 2^-53: the bound of a Cholesky factorisation whose inner products
    have at most w + 1 terms (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.3).  The residual is
    formed in extended precision, so its own rounding does not count."""
    for (name, cfg), (P, r) in built.items():
        if cfg != "host":
            continue
        for q, r0, b, g0, order, w in _blocks(P, r):
            A = _dense_block(P, r0, b, g0)[np.ix_(order, order)]
            L = _dense_factor(r["band%d" % q].reshape(b, w + 1))
            assert np.isfinite(L).all() and (np.diag(L) > 0).all()
            Lx = L.astype(np.longdouble)
            res = np.abs(A.astype(np.longdouble) - Lx @ Lx.T)
            bound = (w + 3) * 2.0 ** -53 * (np.abs(Lx) @ np.abs(Lx).T)
            assert (res <= bound).all(), (name, q, float((res / np.maximum(bound, np.finfo(float).tiny)).max()))


def _window(w):
    W = (w + 64 + 63) & ~63
    if W <= 1024:
        return W
    W = (w + 64 + 127) & ~127
    return W if W <= 2048 else (w + 64 + 255) & ~255


def _reclen(w, wide_from):
    return _window(w) if w > wide_from else (w + 2) & ~1


def test_sweep_records_are_the_documented_formulas(built):
    """invd_f[j] = 1 / L(j,j), forward record of step j: L(j+d, j) * invd_f[j] for d = 1..w; invd_b[j] = 1 / L(jr,jr),
    backward record: L(jr, jr-d) * invd_b[j], jr = b-1-j; slot d-1 of the record (narrow) or (j+d) mod W (wide); one
    reciprocal and one product per value, so equal in bits; every other position zero."""
    seen = set()
    for (name, cfg), (P, r) in built.items():
        if cfg != "host":
            continue
        for q, r0, b, g0, order, w in _blocks(P, r):
            Lb = r["band%d" % q].reshape(b, w + 1)
            wide, rl = w > WIDE_FROM, _reclen(w, WIDE_FROM)
            invf, invb = 1.0 / Lb[:, 0], 1.0 / Lb[::-1, 0]
            assert _same_bits(r["invd_f"][r0:r0 + b], invf) and _same_bits(r["invd_b"][r0:r0 + b], invb)
            f, g = np.zeros((b, rl)), np.zeros((b, rl))
            j = np.arange(b)
            for d in range(1, w + 1):
                slot = (j + d) % rl if wide else np.full(b, d - 1)
                fw = j + d < b                                    # forward: target row j + d exists
                f[j[fw], slot[fw]] = Lb[j[fw] + d, d] * invf[j[fw]]
                jr = b - 1 - j
                bk = jr - d >= 0                                  # backward: target row jr - d exists
                g[j[bk], slot[bk]] = Lb[jr[bk], d] * invb[j[bk]]
            assert _same_bits(r["Lf%d" % q].reshape(b, rl), f), (name, q)
            assert _same_bits(r["Lb%d" % q].reshape(b, rl), g), (name, q)
            seen.add(("wide" if wide else "narrow", "two slabs" if b > 256 else ("ragged" if b % 8 else "even")))
    assert {("narrow", "ragged"), ("narrow", "even"), ("narrow", "two slabs"), ("wide", "ragged"), ("wide", "two slabs")} <= seen


def test_sparse_factored_blocks_get_no_band(exe, tmp_path):
    P = panels()["band"]
    (r,) = run_cases(exe, tmp_path, [block_case(P, 1, 96, nd_mode=2, nd_rows=192)])
    assert int(r["rc"][0]) == OK
    assert list(r["is_nd"]) == [int(b >= 192) for b, _ in BLOCKS]
    for q, r0, b, g0, order, w in _blocks(P, r):
        if r["is_nd"][q]:
            assert "band%d" % q not in r and "coo_off%d" % q not in r
            assert np.array_equal(order, np.arange(b)) and np.array_equal(r["map_b"][r0:r0 + b], np.arange(b)[::-1])
    # mode 1 takes only blocks whose band exceeds 256: none here
    (r,) = run_cases(exe, tmp_path, [block_case(P, 1, 96, nd_mode=1, nd_rows=192)])
    assert not r["is_nd"].any()


def test_a_block_that_is_not_positive_definite_is_named_by_its_row(exe, tmp_path):
    rng = np.random.default_rng(5)
    cases, want = [], []
    for b, w, bad in ((10, 0, 0), (10, 0, 6), (10, 0, 9), (40, 3, 17)):
        L0 = np.tril(rng.uniform(0.25, 1.0, (b, b)), -1) * (np.subtract.outer(np.arange(b), np.arange(b)) <= w) / (w + 1)
        L0 += np.diag(rng.uniform(1.0, 2.0, b))
        A = L0 @ L0.T
        A[bad, bad] = -1.0
        cases.append(cholesky_case(_band_of(A, w)))
        want.append((b, w, bad))
    # through the build: two diagonal blocks, the second with a negative entry; the panel starts at global row 100
    diag = np.arange(1.0, 31.0)
    diag[10 + 7] = -1.0
    P = dict(grow=np.asarray([100, 110, 130], np.int32), rp=np.arange(31, dtype=np.int32), ci=np.arange(100, 130, dtype=np.int32),
             v=diag, row_off=100, m=30, np=2)
    cases.append(block_case(P, 0, 96))
    res = run_cases(exe, tmp_path, cases)
    for (b, w, bad), r in zip(want, res):
        band = r["band"].reshape(b, w + 1)
        assert int(r["bad"][0]) == bad
        assert np.isfinite(band[:bad]).all() and np.isnan(band[bad, 0])
    r = res[-1]
    assert int(r["rc"][0]) == NOT_SPD and int(r["fail_row"][0]) == 117 and int(r["empty"][0]) == 1


# ---- the layout table --------------------------------------------------------------------------------------------
def layout_ref(nrows, bw, is_nd, dev_factor, override, want_g4, want_pairs):
    n = len(nrows)
    L = {}
    wf = FACTOR_WMAX if n < 1024 else 64 * MAX_R - 64
    if override >= 0:
        wf = min(max(override, FACTOR_WMAX), 64 * MAX_R - 64)
    L["wide_from"] = wf
    off, off2, boff = [0], [0] * (n + 1), []
    slist, blist, classes, order = [], [], {}, []
    maxrec = ndev = nnd = btot = 0
    for q in range(n):
        b, w = int(nrows[q]), int(bw[q])
        boff.append(btot)
        if is_nd[q]:
            off.append(off[-1])
            nnd += 1
            continue
        rl = _reclen(w, wf)
        if w <= wf:
            maxrec = max(maxrec, rl)
        ndev += dev_factor
        off.append(off[-1] + b * rl)
        btot += b * (w + 1)
        (slist if w <= FACTOR_WMAX else blist).append(q)
        R = (w + 127) // 64
        if w > wf:
            R = -1 if _window(w) <= 1024 else (-2 if _window(w) <= 2048 else -4)
        if R not in classes:
            classes[R] = []
            order.append(R)
        classes[R].append(q)
    boff.append(btot)
    live = [q for q in range(n) if not is_nd[q]]
    L.update(off=off, tot=off[-1], maxrec=maxrec, pad=256 + 8 * maxrec, ndev=ndev, nnd=nnd, max_bw=max(map(int, bw), default=0),
             boff=boff, btot=btot, slist=slist, ns=len(slist), wsmall=max([int(bw[q]) for q in slist], default=0),
             blist=blist, nbig=len(blist), wbig=max([int(bw[q]) for q in blist], default=0), nclass=len(order), class_R=order,
             class_count=[len(classes[R]) for R in order], class_wmax=[max(int(bw[q]) for q in classes[R]) for R in order],
             class_bmax=[max(int(nrows[q]) for q in classes[R]) for R in order])
    L["class_g4"] = [int(want_g4 and R > 0 and wm <= G4_MAX_BAND and bm <= G4_MAX_ROWS)
                     for R, wm, bm in zip(order, L["class_wmax"], L["class_bmax"])]
    L["class_pairs"] = [int(want_pairs and not g and R in (2, 3)) for R, g in zip(order, L["class_g4"])]
    L["any_g4"], L["any_pairs"] = int(any(L["class_g4"])), int(any(L["class_pairs"]))
    tot2 = 0
    if L["any_g4"] or L["any_pairs"]:
        for q in live:
            if bw[q] <= wf:
                off2[q] = tot2
                tot2 += 8 * ((int(nrows[q]) + 7) // 8) * (int(bw[q]) + 4)
    L.update(off2=off2, tot2=tot2)
    for c, R in enumerate(order):
        L["class_list%d" % c] = classes[R]
    assert max([_window(int(bw[q])) for q in live], default=0) <= 4096
    return L


BWS = [0, 1, 62, 63, 64, 96, 97, 112, 113, 128, 129, 192, 193, 447, 448, 449, 960, 961, 1984, 1985, 4032]
ROWS = [1, 7, 8, 9, 256, 257]


def _layout_inputs():
    """(nrows, bw, is_nd, dev_factor, override, want_g4, want_pairs) over the edges: 1 / 1023 / 1024 blocks, every
    bandwidth and row count of the lists, some blocks sparse, the override absent / below / inside / above its range"""
    out = []
    switches = [(d, o, g, p) for d in (0, 1) for o in (-1, 50, 200, 1000) for g in (0, 1) for p in (0, 1)]
    for n in (1023, 1024):
        q = np.arange(n)
        for rows in (ROWS, ROWS[:-1]):              # with 257 rows in every class bj_g4 takes none
            nrows, bw = np.asarray(rows)[(q // len(BWS) + q) % len(rows)], np.asarray(BWS)[q % len(BWS)]
            out += [(nrows, bw, (q % 11 == 5).astype(int)) + s for s in switches]
    for i, w in enumerate(BWS):                     # one block
        out += [([ROWS[i % 6]], [w], [0]) + s for s in switches[i % 4::4]]
    out.append(([5, 9], [3, 2], [1, 1], 1, -1, 1, 1))          # an all-sparse panel
    return out


def test_layout_table_is_the_restatement(exe, tmp_path):
    inputs = _layout_inputs()
    res = run_cases(exe, tmp_path, [layout_case(*a) for a in inputs])
    seen_g4 = seen_pairs = clamped = 0
    for a, r in zip(inputs, res):
        ref = layout_ref(*a)
        assert int(r["rc"][0]) == OK and len(r["err"]) == 0
        assert set(r) == set(ref) | {"rc", "bad_bw", "err"}
        for k, want in ref.items():
            assert np.array_equal(r[k], np.atleast_1d(np.asarray(want, dtype=r[k].dtype))), (a[3:], k)
        seen_g4 += ref["any_g4"]
        seen_pairs += ref["any_pairs"]
        clamped += a[4] >= 0 and ref["wide_from"] != a[4]
    assert seen_g4 and seen_pairs and clamped
    r = res[-1]
    assert int(r["tot"][0]) == 0 and int(r["nclass"][0]) == 0 and int(r["btot"][0]) == 0 and int(r["nnd"][0]) == 2


def test_layout_refuses_a_band_above_4032(exe, tmp_path):
    ok, bad = run_cases(exe, tmp_path, [layout_case([5000, 9], [4032, 3], [0, 0], 1, -1, 1, 1),
                                        layout_case([9, 5000, 9], [3, 4033, 2], [0, 0, 0], 1, -1, 1, 1)])
    assert int(ok["rc"][0]) == OK and int(ok["max_bw"][0]) == 4032
    assert int(bad["rc"][0]) == BANDWIDTH and int(bad["bad_bw"][0]) == 4033 and int(bad["empty"][0]) == 1
    assert bad["err"].tobytes().decode() == ("block-Jacobi: a diagonal block has bandwidth 4033 after reordering; the "
                                             "workgroup-resident solve supports up to 4032 -- use more (smaller) subdomains")
    # a sparse-factored block of that bandwidth has no window: it is not refused
    (nd,) = run_cases(exe, tmp_path, [layout_case([9, 5000], [3, 4033], [0, 1], 1, -1, 1, 1)])
    assert int(nd["rc"][0]) == OK and int(nd["max_bw"][0]) == 4033
