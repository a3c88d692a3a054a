"""k_coarse_einv_rows (coarse.hip) alone, through its launcher pa_k_coarse_einv_rows(nc, nrows, rows, slab, c, y, ts):
y[rows[x]] = slab[x] . c for the listed rows of the inverse a rank of several keeps.  One process, raw device buffers
through tests/dense_dev.py; slab and c are seeded standard-normal.

Every listed row is held, against a longdouble reference, to (nc + 8) eps sum_j |e_j| |c_j|: one rounding per FMA of the
nc terms, 6 folds across the 64 lanes and 2 across the four wavefronts.  Rows outside the list keep a sentinel in bits,
and two launches agree in bits.  nc = 1, 5 (a row count that is no multiple of the 4 rows of a workgroup), 257 (two
trips of the j loop of 256 lanes) and 1536 (the cap); strides 4, 8 and 16.  Row lists: one row, the last row alone, 5
rows with gaps (as many alternating rows as fit where nc < 9), every row."""
import ctypes as C

import numpy as np
import pytest

from dense_dev import Dev, ci, vp

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    f = d.L.pa_k_coarse_einv_rows
    f.argtypes, f.restype = [ci, ci, vp, vp, vp, vp, ci], ci
    yield d
    d.close()


_ref = {}


def _reference(nc):
    """E (nc x nc), c (nc x 16), and in longdouble E c and |E| |c|: computed once per nc, read by every case."""
    if nc not in _ref:
        rng = np.random.default_rng(1000 + nc)
        E, c = rng.standard_normal((nc, nc)), rng.standard_normal((nc, 16))
        El, cl = E.astype(np.longdouble), c.astype(np.longdouble)
        for a in (E, c):
            a.setflags(write=False)
        _ref[nc] = (E, c, El @ cl, np.abs(El) @ np.abs(cl))
    return _ref[nc]


def _lists(nc):
    gaps = [1, 3, nc // 2, nc - 4, nc - 2] if nc >= 9 else list(range(0, nc, 2))
    return {"one": [min(2, nc - 1)], "last": [nc - 1], "gaps": gaps, "all": list(range(nc))}


@pytest.mark.parametrize("ts", [4, 8, 16])
@pytest.mark.parametrize("nc", [1, 5, 257, 1536])
def test_listed_rows_within_the_bound_the_others_untouched(dev, nc, ts):
    E, c, want, mag = _reference(nc)
    d_c = dev.up(c[:, :ts])
    worst = 0.0
    for name, rows in _lists(nc).items():
        rows = np.asarray(rows, dtype=np.int32)
        assert len(np.unique(rows)) == len(rows) and (np.diff(rows) > 0).all()
        d_rows, d_slab = dev.up(rows), dev.up(E[rows])
        out = []
        for _ in range(2):
            d_y = dev.up(np.full((nc, ts), SENTINEL))
            assert dev.L.pa_k_coarse_einv_rows(nc, len(rows), d_rows, d_slab, d_c, d_y, ts) == 0, dev.error()
            out.append(dev.down(d_y, (nc, ts)))
        y = out[0]
        assert y.tobytes() == out[1].tobytes(), "two launches differ (%s)" % name
        rest = np.ones(nc, dtype=bool)
        rest[rows] = False
        assert y[rest].tobytes() == np.full((int(rest.sum()), ts), SENTINEL).tobytes(), "a row outside the list was written (%s)" % name
        err = np.abs(y[rows].astype(np.longdouble) - want[rows, :ts])
        bound = (nc + 8) * EPS * mag[rows, :ts]
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print("nc %4d ts %2d %-4s: %4d rows, largest error / bound %.3e (error %.3e)" % (nc, ts, name, len(rows), ratio, float(err.max())))
        assert (err <= bound).all(), (name, ratio)
    assert worst < 1.0


def test_the_launcher_refuses_what_it_cannot_run(dev):
    nc, ts = 5, 4
    E, c, _, _ = _reference(nc)
    rows = np.arange(nc, dtype=np.int32)
    d_rows, d_slab, d_c = dev.up(rows), dev.up(E), dev.up(c[:, :ts])
    d_y = dev.up(np.full((nc, ts), SENTINEL))
    f = dev.L.pa_k_coarse_einv_rows
    for args in ((nc, nc, None, d_slab, d_c, d_y, ts), (nc, nc, d_rows, None, d_c, d_y, ts), (nc, nc, d_rows, d_slab, None, d_y, ts),
                 (nc, nc, d_rows, d_slab, d_c, None, ts)):
        assert f(*args) != 0 and "NULL" in dev.error()
    for nrows in (0, -1, nc + 1):
        assert f(nc, nrows, d_rows, d_slab, d_c, d_y, ts) != 0 and "%d rows" % nrows in dev.error()
    assert f(0, 1, d_rows, d_slab, d_c, d_y, ts) != 0
    for bad in (0, 3, 32):
        assert f(nc, nc, d_rows, d_slab, d_c, d_y, bad) != 0 and "stride %d" % bad in dev.error()
    assert dev.down(d_y, (nc, ts)).tobytes() == np.full((nc, ts), SENTINEL).tobytes()       # nothing ran
    assert f(nc, nc, d_rows, d_slab, d_c, d_y, ts) == 0, dev.error()
