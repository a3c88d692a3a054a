"""pa_k_sys_norms_ride (dense_system.hip) alone: the one-workgroup kernel that, with the caller's stopping metric on
several processes, folds this process's sums behind the pair a collective of the iteration carries:
  buf[0] = the scaled sum of squares of all of R, folded from rtr_part as pa_k_group_norms_ride folds it,
  buf[1] = *info,
  buf[2 + j] = the fold of sys_part for system j (one column per system),
and nothing else.  Inputs are random nonnegative partial sums; every output is a fixed-tree sum of n nonnegative terms,
so its relative error against the longdouble sum is at most n u (u = 2^-53; n = k s rtr_nblk for buf[0], sys_nblk for
buf[2 + j]) -- that bound is asserted.  The block counts are 1, 2 and the workgroup size + 1 (a thread of the fold then
takes more than one block, and the last block stands alone in its stride).

The ctypes bindings of the two launchers are this file's own; the device plumbing is tests/dense_dev.py's."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WG = 256
U = 2.0 ** -53
NBLKS = (1, 2, WG + 1)
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def dev():
    from dense_dev import Dev, vp, ci
    d = Dev()
    for name, args in (("pa_k_sys_norms_ride", [vp, ci, vp, ci, ci, ci, ci, vp, vp]),
                       ("pa_k_group_norms_ride", [vp, ci, ci, ci, ci, vp, vp])):
        f = getattr(d.L, name)
        f.argtypes, f.restype = args, ci
    yield d
    d.close()


def _cases(ts):
    return [(k, s) for k, s in ((1, 4), (4, 1), (2, 2), (3, 1), (16, 1)) if k * s <= ts and ((k, s) != (3, 1) or ts == 4)]


@pytest.mark.parametrize("ts", [4, 8, 16])
def test_the_folds_meet_the_bound_and_write_nothing_else(dev, ts):
    rng = np.random.default_rng(20261020 + ts)
    L = dev.L
    assert _cases(ts)
    for (k, s), rtr_nblk, sys_nblk in itertools.product(_cases(ts), NBLKS, NBLKS):
        # partial sums of squares: nonnegative, spread over twelve orders of magnitude; every column of the stride is
        # filled, so a fold that read beyond its k s (or k) columns would show
        rtr = rng.random((rtr_nblk, ts)) * 10.0 ** rng.uniform(-6, 6, (rtr_nblk, ts))
        sysp = rng.random((sys_nblk, ts)) * 10.0 ** rng.uniform(-6, 6, (sys_nblk, ts))
        info = 3 + k
        d_rtr, d_sys = dev.up(rtr), dev.up(sysp)
        d_info = dev.up(np.array([info, 0], dtype=np.int32))
        room = 2 + 2 + 16 + 2                  # two sentinels in front, the words, sentinels behind
        outs = []
        for _ in range(2):
            d_buf = dev.up(np.full(room, SENTINEL))
            dev.check(L.pa_k_sys_norms_ride(d_rtr, rtr_nblk, d_sys, sys_nblk, ts, k, s, d_info, d_buf + 16), "ride")
            outs.append(dev.down(d_buf, (room,)))
        got = outs[0]
        assert outs[1].tobytes() == got.tobytes(), "two launches differ"
        buf = got[2:]
        assert (got[:2] == SENTINEL).all() and (buf[2 + k:] == SENTINEL).all(), (k, s, got)
        assert buf[1] == float(info)
        want0 = rtr[:, :k * s].astype(np.longdouble).sum()
        n0 = k * s * rtr_nblk
        assert abs(buf[0] - want0) <= n0 * U * want0, ((k, s), rtr_nblk, float(abs(buf[0] - want0) / want0), n0 * U)
        for j in range(k):
            want = sysp[:, j].astype(np.longdouble).sum()
            assert abs(buf[2 + j] - want) <= sys_nblk * U * want, ((k, s), sys_nblk, j, float(abs(buf[2 + j] - want) / want))
        # buf[0] has the bits pa_k_group_norms_ride gives on the same column sums
        d_ref = dev.up(np.full(2 + 16, SENTINEL))
        dev.check(L.pa_k_group_norms_ride(d_rtr, rtr_nblk, ts, k, s, d_info, d_ref), "group ride")
        ref = dev.down(d_ref, (2 + 16,))
        assert ref[0].tobytes() == buf[0].tobytes() and ref[1] == buf[1], ((k, s), rtr_nblk, ref[0], buf[0])
        # info == NULL: status 0
        d_buf = dev.up(np.full(room, SENTINEL))
        dev.check(L.pa_k_sys_norms_ride(d_rtr, rtr_nblk, d_sys, sys_nblk, ts, k, s, None, d_buf + 16), "ride")
        nul = dev.down(d_buf, (room,))
        assert nul[3] == 0.0 and nul[2].tobytes() == buf[0].tobytes() and nul[4:4 + k].tobytes() == buf[2:2 + k].tobytes()
        dev.close()


def test_the_launcher_refuses_what_does_not_fit_and_a_missing_buffer(dev):
    L = dev.L
    d_part = dev.up(np.ones((2, 4)))
    d_buf = dev.up(np.full(8, SENTINEL))
    assert L.pa_k_sys_norms_ride(d_part, 2, d_part, 2, 4, 3, 2, None, d_buf) == 1
    assert "pa_k_sys_norms_ride" in dev.error() and "3 systems of 2 columns do not fit a panel of stride 4" in dev.error()
    assert L.pa_k_sys_norms_ride(d_part, 2, d_part, 2, 4, 2, 2, None, None) == 1
    assert "pa_k_sys_norms_ride: no buffer for the 2 sums" in dev.error()
    assert (dev.down(d_buf, (8,)) == SENTINEL).all()
    dev.close()
