"""The MatrixMarket reader (prealps_amd/csrc/mtx_read.c) alone: a stand-alone program (tests/c/mtx_read_check.c) links
the unit, is compiled with AddressSanitizer + UBSan and run as a program.  No scaling is involved here, so a good file
must give scipy's matrix exactly (repeated entries: summed in file order); a bad file its message, an empty result and
no leak.  tests/test_mtx_reader_cpu.py checks the same styles through the whole library."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prealps_amd", "csrc")
HEAD = "%%MatrixMarket matrix coordinate real general\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is needed to build tests/c/mtx_read_check.c")
    tmp = tmp_path_factory.mktemp("mtx_read")
    out, unit = str(tmp / "mtx_read_check"), str(tmp / "mtx_read.o")
    flags = ["-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC]
    subprocess.check_call([gcc] + flags + ["-c", os.path.join(CSRC, "mtx_read.c"), "-o", unit])
    subprocess.check_call([gcc] + flags + [os.path.join(ROOT, "tests", "c", "mtx_read_check.c"), unit, "-o", out])
    return out


def run(exe, path, threads):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, path, str(threads)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", "sanitizer or program failure:\n" + r.stderr[-4000:]
    return r.stdout


def read(exe, path):
    out = run(exe, path, 1)
    assert out == run(exe, path, 4)                  # the number of threads changes nothing
    lines = dict(line.split(" ", 1) for line in out.splitlines())
    assert "error" not in lines, lines
    arr = lambda name, dt: np.array(lines[name].split()[1:], dtype=dt)
    n = int(lines["N"])
    return sp.csr_matrix((arr("val", np.float64), arr("colInd", np.int64), arr("rowPtr", np.int64)), shape=(n, n))


def test_the_unit_includes_its_own_header_the_allocation_header_and_libc_only():
    src = open(os.path.join(CSRC, "mtx_read.c")).read() + open(os.path.join(CSRC, "mtx_read.h")).read()
    includes = set(line.split()[1] for line in src.splitlines() if line.startswith("#include"))
    assert includes == {'"mtx_read.h"', '"pa_alloc.h"', "<omp.h>", "<stddef.h>", "<stdio.h>", "<stdlib.h>", "<string.h>",
                        "<strings.h>", "<sys/mman.h>"}
    assert "getenv" not in src and "pa_host" not in src and "PA_FAIL" not in src


def _spd(n, seed, density=0.01):
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=rng, format="csr")
    A = M + M.T
    return sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0))


def _same(got, ref):
    ref = sp.csr_matrix(ref); ref.sort_indices()
    np.testing.assert_array_equal(got.indptr, ref.indptr)
    np.testing.assert_array_equal(got.indices, ref.indices)       # columns ascending in every row
    assert np.array_equal(got.data, ref.data)                     # the doubles, by ==


@pytest.mark.parametrize("style", ["general", "symmetric", "zero_based", "crlf_blank_no_final_newline", "duplicates", "comments_in_body"])
def test_reader_gives_scipys_matrix(exe, tmp_path, style):
    A = _spd(300, 1)
    coo = sp.coo_matrix(A)
    rows, cols, vals = coo.row, coo.col, coo.data
    sym, base, eol = False, 1, "\n"
    ref = A
    if style == "symmetric":
        keep = rows >= cols
        rows, cols, vals, sym = rows[keep], cols[keep], vals[keep], True
    if style == "zero_based":
        base = 0
        order = np.lexsort((cols, rows))          # the reference decides on the FIRST entry: make it (0, 0)
        rows, cols, vals = rows[order], cols[order], vals[order]
    if style == "crlf_blank_no_final_newline":
        eol = "\r\n"
    if style == "duplicates":                      # every entry split into two parts, summed in file order: first + second
        ref = sp.csr_matrix((0.25 * vals + 0.75 * vals, (rows, cols)), shape=A.shape)
        rows, cols, vals = np.concatenate([rows, rows]), np.concatenate([cols, cols]), np.concatenate([0.25 * vals, 0.75 * vals])
    path = str(tmp_path / "a.mtx")
    with open(path, "w", newline="") as f:
        f.write("%%%%MatrixMarket matrix coordinate real %s%s" % ("symmetric" if sym else "general", eol))
        f.write("% a comment" + eol)
        f.write("%d %d %d%s" % (A.shape[0], A.shape[1], len(vals), eol))
        lines = ["%d %d %.17g" % (r + base, c + base, x) for r, c, x in zip(rows, cols, vals)]
        if style == "comments_in_body":            # '%' lines between the entries: skipped, not counted
            lines.insert(3, "% a remark in the middle")
            lines.insert(40, "  % and an indented one")
            lines.append("% and one at the end")
        if style == "crlf_blank_no_final_newline":
            lines.insert(5, "")
            f.write(eol.join(lines))
        else:
            f.write(eol.join(lines) + eol)
    _same(read(exe, path), ref)


def test_reader_on_a_file_cut_into_a_piece_per_thread(exe, tmp_path):
    """More than 4096 entries per thread, in no particular order: every thread parses a piece of its own."""
    n = 3000
    A = _spd(n, 7, density=0.002)
    coo = sp.coo_matrix(sp.tril(A))
    assert coo.nnz > 4 * 4096
    perm = np.random.default_rng(3).permutation(coo.nnz)
    path = str(tmp_path / "big.mtx")
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real symmetric\n%d %d %d\n" % (n, n, coo.nnz))
        np.savetxt(f, np.column_stack([coo.row[perm] + 1, coo.col[perm] + 1, coo.data[perm]]), fmt="%d %d %.17g")
    _same(read(exe, path), A)


def test_reader_refuses_bad_files(exe, tmp_path):
    cases = [(HEAD + "3 3 3\n1 1 1.0\n2 2 1.0\n", "bad entry 2 in %s"),
             (HEAD + "3 3 3\n1 1 1.0\n2 x 1.0\n3 3 1.0\n", "bad entry 1 in %s"),
             (HEAD + "3 3 3\n1 1 1.0\n2 2 1.0\n4 3 1.0\n", "index out of range in %s"),
             ("%%MatrixMarket matrix array real general\n3 3\n",
              "Only sparse real < symmetric | general > matrix are currently supported (%s)"),
             (None, "Impossible to open the file %s"),                                   # a missing file
             (HEAD + "% cut off inside the header\n", "truncated file %s"),
             (HEAD + "3 4 3\n1 1 1.0\n", "[LoadMatrixMarket] Error: Invalid matrix dimensions in %s")]
    for i, (body, msg) in enumerate(cases):
        p = str(tmp_path / ("bad%d.mtx" % i))
        if body is not None:
            open(p, "w").write(body)
        for threads in (1, 4):
            lines = dict(line.split(" ", 1) for line in run(exe, p, threads).splitlines())
            code, _, text = lines["error"].partition(" ")
            assert int(code) != 0 and text == msg % p and lines["empty"] == "1", lines
