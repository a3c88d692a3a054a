"""The class pass of the block-Jacobi create (prealps_amd/csrc/bj_share.c): which diagonal blocks have the same rows,
the same bandwidth and the same band, bit for bit, so that the apply may read one block's records for all of them.
tests/c/bj_share_check.c, a stand-alone program built with AddressSanitizer + UBSan together with bj_share.c alone,
runs the unit on the cases written here; rep[] is compared with a numpy restatement of the rule: the first index of
each distinct (nrows, bw, band bytes) among the eligible blocks, the block itself otherwise.

Every set of blocks runs with the full hash, with a one-bit hash and with no hash at all (hash_mask 0: every block
collides with every other, the forced collision of equal hash and different bytes), on one and on three threads: the
hash may only find candidates, so the classes are the same six times."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
FULL = 2 ** 64 - 1
MASKS = (FULL, 1, 0)


def share_case(blocks, threads, mask):
    """blocks: (nrows, bw, eligible, band or None)"""
    n = len(blocks)
    out = [np.asarray([n, threads], np.int32).tobytes(), struct.pack("<Q", mask)]
    out += [np.asarray([b[k] for b in blocks], np.int32).tobytes() for k in (0, 1, 2)]
    out.append(np.asarray([b[3] is not None for b in blocks], np.int32).tobytes())
    for b, w, _, band in blocks:
        if band is not None:
            band = np.ascontiguousarray(band, np.float64)
            assert band.size == b * (w + 1)
            out.append(band.tobytes())
    return b"".join(out)


def rep_ref(blocks):
    seen, rep = {}, []
    for p, (b, w, el, band) in enumerate(blocks):
        if not el or band is None:
            rep.append(p)
            continue
        rep.append(seen.setdefault((b, w, np.ascontiguousarray(band, np.float64).tobytes()), p))
    return rep


def read_arrays(path):
    out, kinds = {}, {"i": np.int32, "q": np.int64}
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
        pytest.fail("gcc is needed to build tests/c/bj_share_check.c")
    tmp = tmp_path_factory.mktemp("bj_share")
    exe, unit = str(tmp / "bj_share_check"), str(tmp / "bj_share.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "bj_share.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "bj_share_check.c"), unit, "-o", exe])
    return exe


def run_sets(exe, tmp, sets):
    """every set of blocks under every mask and thread count; returns the rep[] all six runs agree on, per set"""
    variants = [(t, m) for t in (1, 3) for m in MASKS]
    src, dst = os.path.join(str(tmp), "cases.bin"), os.path.join(str(tmp), "arrays.bin")
    with open(src, "wb") as f:
        f.write(b"".join(share_case(blocks, t, m) for blocks in sets for t, m in variants))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    out = read_arrays(dst)
    assert sorted(out) == list(range(len(sets) * len(variants)))
    reps = []
    for i, blocks in enumerate(sets):
        got = [out[i * len(variants) + v] for v in range(len(variants))]
        for g, v in zip(got, variants):
            assert int(g["rc"][0]) == 0, v
            assert np.array_equal(g["rep"], got[0]["rep"]), (i, v)
            assert int(g["nclass"][0]) == int(np.count_nonzero(g["rep"] == np.arange(len(blocks)))), (i, v)
        reps.append([int(r) for r in got[0]["rep"]])
    return reps


def _band(rng, b, w):
    return rng.standard_normal((b, w + 1))


def _bump(band, at=-1):
    """the same band but for the last place of one value"""
    c = np.array(band, np.float64)
    flat = c.reshape(-1).view(np.uint64)
    flat[at] ^= np.uint64(1)
    return c


def test_equal_blocks_share_the_lowest_numbered_one(exe, tmp_path):
    rng = np.random.default_rng(1)
    a, b, c = _band(rng, 40, 7), _band(rng, 40, 7), _band(rng, 17, 0)
    blocks = [(40, 7, 1, x) for x in (a, b, a, a, b)] + [(17, 0, 1, c), (40, 7, 1, a.copy()), (17, 0, 1, c)]
    (rep,) = run_sets(exe, tmp_path, [blocks])
    assert rep == rep_ref(blocks) == [0, 1, 0, 0, 1, 5, 0, 5]


def test_one_bit_a_signed_zero_a_bandwidth_or_a_row_count_keep_blocks_apart(exe, tmp_path):
    rng = np.random.default_rng(2)
    a = _band(rng, 12, 2)
    z = a.copy()
    z[5, 1] = 0.0
    zn = z.copy()
    zn[5, 1] = -0.0
    nan = a.copy()
    nan[3, 0] = np.nan
    nan2 = nan.copy()
    nan2.reshape(-1).view(np.uint64)[3 * 3] ^= np.uint64(1)              # another NaN: other payload bits
    assert np.isnan(nan2[3, 0]) and nan.tobytes() != nan2.tobytes()
    twelve = rng.standard_normal(12)
    sets = [
        [(12, 2, 1, a), (12, 2, 1, _bump(a)), (12, 2, 1, _bump(a, 0)), (12, 2, 1, a), (12, 2, 1, _bump(a))],
        [(12, 2, 1, z), (12, 2, 1, zn), (12, 2, 1, z), (12, 2, 1, zn)],
        [(12, 2, 1, nan), (12, 2, 1, nan2), (12, 2, 1, nan), (12, 2, 1, nan2)],
        # the same 96 bytes as four shapes: bw and nrows belong to the key
        [(12, 0, 1, twelve), (6, 1, 1, twelve), (4, 2, 1, twelve), (3, 3, 1, twelve), (6, 1, 1, twelve), (12, 0, 1, twelve)],
        # the same rows, another bandwidth: one band is the other with a zero column more
        [(5, 1, 1, a[:5, :2]), (5, 2, 1, np.hstack([a[:5, :2], np.zeros((5, 1))])), (5, 1, 1, a[:5, :2])],
    ]
    reps = run_sets(exe, tmp_path, sets)
    assert reps == [rep_ref(s) for s in sets]
    assert reps == [[0, 1, 2, 0, 1], [0, 1, 0, 1], [0, 1, 0, 1], [0, 1, 2, 3, 1, 0], [0, 1, 0]]


def test_a_block_that_is_not_eligible_shares_nothing_and_hides_nothing(exe, tmp_path):
    rng = np.random.default_rng(3)
    a = _band(rng, 9, 4)
    sets = [[(9, 4, 1, a), (9, 4, 0, a), (9, 4, 1, a)],           # the same bytes, but not eligible
            [(9, 4, 1, a), (9, 4, 0, None), (9, 4, 1, a)],        # no band at all (a wide or a sparse-factored block)
            [(9, 4, 0, a), (9, 4, 1, a), (9, 4, 1, a)],           # the lowest-numbered ELIGIBLE block represents
            [(9, 4, 0, None), (9, 4, 0, a), (9, 4, 0, a)]]
    reps = run_sets(exe, tmp_path, sets)
    assert reps == [rep_ref(s) for s in sets] == [[0, 1, 0], [0, 1, 0], [0, 1, 1], [0, 1, 2]]


def test_smallest_inputs(exe, tmp_path):
    one = np.asarray([[2.5]])
    sets = [[(1, 0, 1, one)],                                                   # np = 1
            [(7, 3, 0, None)],
            [(1, 0, 1, one), (1, 0, 1, one), (1, 0, 1, _bump(one)), (1, 0, 1, one)],      # b = 1 with w = 0
            []]
    reps = run_sets(exe, tmp_path, sets)
    assert reps == [rep_ref(s) for s in sets] == [[0], [0], [0, 0, 2, 0], []]


def test_many_blocks_in_few_classes(exe, tmp_path):
    """300 blocks of six shapes drawn from 14 distinct bands, in random order: the restatement, and with no hash at
    all every block is a candidate of every representative of its shape."""
    rng = np.random.default_rng(4)
    shapes = [(1, 0), (5, 0), (16, 15), (17, 5), (64, 33), (65, 64)]
    pool = []
    for b, w in shapes:
        base = _band(rng, b, w)
        pool += [(b, w, base), (b, w, _bump(base))]
    pool += [(64, 33, _band(rng, 64, 33)), (17, 5, _band(rng, 17, 5))]
    pick = rng.integers(0, len(pool), 300)
    blocks = [(pool[k][0], pool[k][1], int(i % 13 != 5), pool[k][2]) for i, k in enumerate(pick)]
    (rep,) = run_sets(exe, tmp_path, [blocks])
    assert rep == rep_ref(blocks)
    assert len({r for r, b in zip(rep, blocks) if b[2]}) == len({int(k) for k, b in zip(pick, blocks) if b[2]})
