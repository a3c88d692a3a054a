"""The pair tasks of the block-Jacobi create (prealps_amd/csrc/bj_share.c: pa_bj_pair_tasks): which two blocks of a
launch list share a wavefront of the PAIR launch of bj_g4.hip.  tests/c/bj_pair_check.c, a stand-alone program built
with AddressSanitizer + UBSan together with bj_share.c alone, runs the builder on the cases written here; the tasks are
compared with a numpy restatement of the rule -- the positions of a class (equal rep) in list order, first with second,
third with fourth, a last odd one alone, tasks sorted by their first position -- and checked on their own: every
position exactly once, partners of one class with equal rows and bandwidth, i0 < i1, ascending i0."""
import os
import shutil
import signal
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")


def pair_case(rep, nrows, bw, lst):
    rep, nrows, bw, lst = (np.asarray(a, np.int32) for a in (rep, nrows, bw, lst))
    assert len(rep) == len(nrows) == len(bw)
    return b"".join([np.asarray([len(rep), len(lst)], np.int32).tobytes(), rep.tobytes(), nrows.tobytes(), bw.tobytes(),
                     lst.tobytes()])


def tasks_ref(rep, lst):
    """numpy restatement: (i0, i1) rows, i1 = -1 without a partner"""
    lst = np.asarray(lst, np.int64)
    if lst.size == 0:
        return np.zeros((0, 2), np.int64)
    cls = np.asarray(rep, np.int64)[lst]
    out = []
    for c in np.unique(cls):
        pos = np.nonzero(cls == c)[0]                       # ascending: list order
        pad = np.concatenate([pos, [-1] * (pos.size % 2)])
        out.append(pad.reshape(-1, 2))
    out = np.concatenate(out)
    return out[np.argsort(out[:, 0], kind="stable")]


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
        pytest.fail("gcc is needed to build tests/c/bj_pair_check.c")
    tmp = tmp_path_factory.mktemp("bj_pair")
    exe, unit = str(tmp / "bj_pair_check"), str(tmp / "bj_share.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "bj_share.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "bj_pair_check.c"), unit, "-o", exe])
    return exe


def _run(exe, tmp, cases):
    src, dst = os.path.join(str(tmp), "cases.bin"), os.path.join(str(tmp), "arrays.bin")
    with open(src, "wb") as f:
        f.write(b"".join(pair_case(*c) for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    return run, (read_arrays(dst) if os.path.exists(dst) else {})


def run_cases(exe, tmp, cases):
    """cases: (rep, nrows, bw, list); returns the (ntasks, 2) tasks of each, checked"""
    run, out = _run(exe, tmp, cases)
    assert run.returncode == 0 and run.stderr == "", "sanitizer or program failure:\n" + run.stdout[-2000:] + run.stderr[-4000:]
    assert sorted(out) == list(range(len(cases)))
    res = []
    for i, (rep, nrows, bw, lst) in enumerate(cases):
        g = out[i]
        nt, paired = int(g["ntasks"][0]), int(g["paired"][0])
        assert int(g["rc"][0]) == 0 and g["tasks"].size == 2 * nt
        t = g["tasks"].reshape(-1, 2).astype(np.int64)
        ref = tasks_ref(rep, lst)
        assert np.array_equal(t, ref), (i, t.tolist(), ref.tolist())
        # ... and on their own terms
        used = np.concatenate([t[:, 0], t[t[:, 1] >= 0, 1]])
        assert sorted(used.tolist()) == list(range(len(lst))), i                  # every position exactly once
        assert np.all(np.diff(t[:, 0]) > 0)                                          # ordered by i0
        assert paired == 2 * int(np.count_nonzero(t[:, 1] >= 0))
        for i0, i1 in t[t[:, 1] >= 0]:
            p0, p1 = lst[i0], lst[i1]
            assert i0 < i1 and rep[p0] == rep[p1] and nrows[p0] == nrows[p1] and bw[p0] == bw[p1], (i, i0, i1)
        # a class's pairs in list order: the k-th pair holds its positions 2 k and 2 k + 1
        cls = np.asarray(rep)[np.asarray(lst, np.int64)] if len(lst) else np.zeros(0, np.int64)
        for c in np.unique(cls):
            pos = np.nonzero(cls == c)[0]
            mine = t[np.isin(t[:, 0], pos)]
            assert mine[:, 0].tolist() == pos[0::2].tolist()
            assert mine[:, 1].tolist() == pos[1::2].tolist() + [-1] * (pos.size % 2)
        res.append(t)
    return res


def _shape(rep, rows=(40, 17, 9, 192), bands=(7, 0, 4, 64)):
    """rows and bandwidth that go with a rep[]: one shape per class"""
    rep = np.asarray(rep)
    return rep, np.asarray(rows)[rep % len(rows)], np.asarray(bands)[rep % len(bands)]


def test_classes_of_one_two_three_and_five_members(exe, tmp_path):
    #         0  1  2  3  4  5  6  7  8  9 10
    rep = [0, 1, 1, 3, 3, 3, 6, 6, 6, 6, 6]
    r, nr, bw = _shape(rep)
    lst = list(range(11))
    (t,) = run_cases(exe, tmp_path, [(r, nr, bw, lst)])
    assert t.tolist() == [[0, -1], [1, 2], [3, 4], [5, -1], [6, 7], [8, 9], [10, -1]]


def test_members_interleaved_with_other_classes(exe, tmp_path):
    rep = [0, 1, 0, 1, 0, 5, 1, 0, 5, 0, 1]
    r, nr, bw = _shape(rep)
    lst = list(range(11))
    (t,) = run_cases(exe, tmp_path, [(r, nr, bw, lst)])
    assert t.tolist() == [[0, 2], [1, 3], [4, 7], [5, 8], [6, 10], [9, -1]]


def test_blocks_that_are_not_eligible_stand_alone_in_between(exe, tmp_path):
    """a block that may not share is its own class (rep[p] = p) whatever its shape: it pairs with nobody and does not
    keep the members around it apart"""
    rep = [0, 1, 0, 3, 0, 5, 0]
    nrows, bw = [40] * 7, [7] * 7                              # all of one shape: only rep decides
    (t,) = run_cases(exe, tmp_path, [(rep, nrows, bw, list(range(7)))])
    assert t.tolist() == [[0, 2], [1, -1], [3, -1], [4, 6], [5, -1]]


def test_a_list_that_is_a_class_of_the_layout(exe, tmp_path):
    """the list holds some of the blocks, in its own order: the tasks are positions into the LIST"""
    rep = [0, 0, 2, 0, 2, 5, 0, 2, 0, 5]
    r, nr, bw = _shape(rep)
    lists = [[9, 8, 6, 5, 3, 1, 0], [2, 4, 7], [7, 0], [4, 7, 2, 1]]
    ts = run_cases(exe, tmp_path, [(r, nr, bw, lst) for lst in lists])
    assert ts[0].tolist() == [[0, 3], [1, 2], [4, 5], [6, -1]]
    assert ts[1].tolist() == [[0, 1], [2, -1]]
    assert ts[2].tolist() == [[0, -1], [1, -1]]
    assert ts[3].tolist() == [[0, 1], [2, -1], [3, -1]]


def test_smallest_inputs(exe, tmp_path):
    cases = [([0], [5], [2], [0]),                    # np = 1
             ([0], [5], [2], []),                     # np = 1, an empty list
             ([], [], [], []),                        # nothing at all
             ([0, 0], [1, 1], [0, 0], [1, 0])]        # one pair of one-row blocks, listed backwards
    ts = run_cases(exe, tmp_path, cases)
    assert [t.tolist() for t in ts] == [[[0, -1]], [], [], [[0, 1]]]


def test_many_blocks_in_few_classes(exe, tmp_path):
    rng = np.random.default_rng(7)
    np_ = 400
    first = rng.integers(0, 12, np_)
    rep = np.asarray([int(np.nonzero(first == f)[0][0]) for f in first])
    rep[::13] = np.arange(np_)[::13]                                 # some that may not share ...
    for p in range(np_):                                             # ... and nobody reads their records
        if rep[rep[p]] != rep[p]:
            rep[p] = p
    r, nr, bw = _shape(rep)
    lst = rng.permutation(np_)[:333]
    (t,) = run_cases(exe, tmp_path, [(r, nr, bw, lst.tolist())])
    assert 0 < np.count_nonzero(t[:, 1] < 0) < len(t)


def test_equal_rep_with_unequal_rows_or_band_is_refused_by_assertion(exe, tmp_path):
    """blocks of one class have the same rows and bandwidth by construction (bj_share.h); the builder asserts it"""
    for nrows, bw in (([40, 41], [7, 7]), ([40, 40], [7, 6])):
        run, _ = _run(exe, tmp_path, [([0, 0], nrows, bw, [0, 1])])
        assert run.returncode == -signal.SIGABRT, (run.returncode, run.stderr[-2000:])
        assert "Assertion" in run.stderr and "pa_bj_pair_tasks" in run.stderr
