"""The solution history on several processes, the device side alone: the launchers of prealps_amd/csrc/history.hip that
work on the rows a process owns (pa_k_hist_gather, pa_k_hist_ring_scaled, pa_k_hist_project_owned, pa_k_hist_gram_owned,
pa_k_hist_combine_owned) through ctypes against long double, shaped like
tests/test_gpu_solution_history.py::test_kernels_against_long_double.

The ring Xl holds m rows (local row r is the caller's row src[r] of N = m + 37, src a shuffled m-subset); the caller's
arrays have N rows and NaN in every row the process does not own, in the padding rows and in the dead slots of the ring, so
a read outside the owned rows shows in the sums.  Bounds: tests/history_ref.py (they hold for any order of summation);
the mapped Gram blocks take gamma(m + 2) |X|^T |W / dl| as the existing mapped dots do (m products, one division, the
sums).  The offsets into the collective buffer are restated here (ecg_history.h: pa_hist_red_layout): the sums b_j^2 at
word 1, g and DO at word 17, DN at word 273.  One pair of other offsets is run as well: the fold goes where it is told."""
import ctypes as C

import numpy as np
import pytest

import history_ref as H

pytestmark = pytest.mark.gpu

LD = np.longdouble
vp, ci = C.c_void_p, C.c_int
RED_WORDS = 1 + 16 + 256 + 256
SENTINEL = -12345.678


class Dev:
    def __init__(self):
        import prealps_amd
        from prealps_amd.lib import check
        self.L, self.check = prealps_amd.load(), check
        L = self.L
        check(L.preAlps_hip_init(0), "init")
        L.pa_rt_error.restype = C.c_char_p
        L.pa_rt_malloc.restype, L.pa_rt_malloc.argtypes = vp, [C.c_size_t]
        L.pa_rt_free.restype, L.pa_rt_free.argtypes = None, [vp]
        L.pa_rt_h2d.argtypes = [vp, vp, C.c_size_t]
        L.pa_rt_d2h.argtypes = [vp, vp, C.c_size_t]
        L.pa_k_hist_owned_part_doubles.restype = C.c_size_t
        L.pa_k_hist_gather.argtypes = [ci, ci, ci, vp, vp, ci, vp, ci, vp, ci]
        L.pa_k_hist_ring_scaled.argtypes = [ci, ci, vp, ci, vp, vp, ci]
        L.pa_k_hist_project_owned.argtypes = [ci, ci, ci, ci, vp, ci, ci, ci, vp, vp, ci, vp, vp, ci, ci]
        L.pa_k_hist_gram_owned.argtypes = [ci, ci, ci, vp, ci, ci, ci, vp, ci, vp, vp, ci, vp, vp, ci, ci]
        L.pa_k_hist_combine_owned.argtypes = [ci, ci, ci, ci, vp, ci, ci, ci, vp, vp, vp, ci]
        L.pa_k_hist_combine.argtypes = [ci, ci, ci, vp, ci, ci, ci, vp, vp, ci]
        self.bufs = []
        self.part = self.alloc(L.pa_k_hist_owned_part_doubles() * 8)

    def alloc(self, nbytes):
        d = self.L.pa_rt_malloc(max(nbytes, 8))
        assert d
        self.bufs.append(d)
        return d

    def up(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        self.check(self.L.pa_rt_h2d(d, a.ctypes.data, a.nbytes), "h2d")
        return d

    def down(self, d, n):
        h = np.zeros(n)
        self.check(self.L.preAlps_hip_sync(), "sync")
        self.check(self.L.pa_rt_d2h(h.ctypes.data, d, h.nbytes), "d2h")
        return h

    def free_all_but_part(self):
        self.L.preAlps_hip_sync()
        for d in self.bufs[1:]:
            self.L.pa_rt_free(d)
        self.bufs = self.bufs[:1]

    def close(self):
        self.L.preAlps_hip_sync()
        for d in self.bufs:
            self.L.pa_rt_free(d)
        self.bufs = []


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def _colmajor(V, ld):
    """The (n, k) array V as k columns of ld doubles, NaN in the padding rows."""
    out = np.full((V.shape[1], ld), np.nan)
    out[:, :V.shape[0]] = V.T
    return out


def _global(V, src, N, ld):
    """The m owned rows V spread over the caller's N rows (k columns of ld doubles): NaN everywhere else."""
    out = np.full((V.shape[1], ld), np.nan)
    out[:, src] = V.T
    return out


def _twice(dev, launch, d_out, n):
    got = []
    for _ in range(2):
        assert launch() == 0, dev.L.pa_rt_error()
        got.append(dev.down(d_out, n))
    assert got[0].tobytes() == got[1].tobytes()
    return got[0]


def _outside(red, blocks):
    """The words of the collective buffer outside the given (offset, count) blocks."""
    keep = np.ones(RED_WORDS, dtype=bool)
    for off, n in blocks:
        keep[off:off + n] = False
    return red[keep]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000, 4097])
def test_owned_kernels_against_long_double(dev, m):
    rng = np.random.default_rng(m)
    L = dev.L
    N = m + 37
    case = 0
    for K in (1, 3, 4, 5, 8, 16):
        for q in (1, 2, 4, 5, 16):
            case += 1
            ldh = m + (3 if case % 2 else 0)            # the ring's leading dimension: local rows
            ldg = N + (5 if case % 2 else 0)            # the caller's arrays: global rows
            cap = min(16, K + case % 3)
            head = (case * 5) % cap                     # a ring that has wrapped whenever head > 0
            src = rng.permutation(N)[:m].astype(np.int32)
            dl = rng.uniform(0.5, 2.0, m)
            X = rng.standard_normal((m, K))
            ring = np.full((m, cap), np.nan)            # slots that hold no live column: NaN
            for i in range(K):
                ring[:, (head + i) % cap] = X[:, i]
            d_src, d_dl, d_ring = dev.up(src), dev.up(dl), dev.up(_colmajor(ring, ldh))

            # ---- the projection's dots: g = Xl^T b[src] and the sums b_j^2, b read through src ----
            Bo = rng.standard_normal((m, q))
            d_b = dev.up(_global(Bo, src, N, ldg))
            d_red = dev.up(np.full(RED_WORDS, SENTINEL))
            off_bb, off_g = (1, 17) if case % 4 else (1 + K * q, 1)
            red = _twice(dev, lambda: L.pa_k_hist_project_owned(m, N, K, q, d_ring, ldh, head, cap, d_src, d_b, ldg, dev.part,
                                                                d_red, off_bb, off_g), d_red, RED_WORDS)
            g = red[off_g:off_g + K * q].reshape(q, K).T
            assert (np.abs(g - H.dots_exact(X, Bo)) <= H.dots_bound(X, Bo, m)).all(), (K, q)
            b2 = red[off_bb:off_bb + q]
            exact = (Bo.astype(LD) ** 2).sum(axis=0)
            assert (np.abs(b2 - exact) <= H.gamma(m) * exact).all(), (K, q)
            assert (_outside(red, [(off_bb, q), (off_g, K * q)]) == SENTINEL).all(), (K, q)     # word 0 among them

            # ---- the Gram blocks: DO = Xl^T (W / dl), DN = Xn^T (W / dl), W a row-major panel ----
            ts = next(t for t in (2, 4, 8, 16) if t >= q)
            W = rng.standard_normal((m, q))
            Xn = rng.standard_normal((m, q))
            panel = np.full((m, ts), np.nan)
            panel[:, :q] = W
            d_panel, d_xn = dev.up(panel), dev.up(_colmajor(Xn, ldh))
            d_red = dev.up(np.full(RED_WORDS, SENTINEL))
            off_do, off_dn = (17, 273) if case % 4 else (1 + q * q, 1)
            red = _twice(dev, lambda: L.pa_k_hist_gram_owned(m, K, q, d_ring, ldh, head, cap, d_xn, ldh, d_dl, d_panel, ts,
                                                             dev.part, d_red, off_do, off_dn), d_red, RED_WORDS)
            Wd = W.astype(LD) / dl.astype(LD)[:, None]
            for left, off, rows in ((X, off_do, K), (Xn, off_dn, q)):
                got = red[off:off + rows * q].reshape(q, rows).T
                bound = H.gamma(m + 2) * (np.abs(left).astype(LD).T @ np.abs(Wd))
                assert (np.abs(got - left.astype(LD).T @ Wd) <= bound).all(), (K, q, off)
            assert (_outside(red, [(off_do, K * q), (off_dn, q * q)]) == SENTINEL).all(), (K, q)
            # the ring alone (the refresh): the same DO, and the block behind it is left alone
            d_red2 = dev.up(np.full(RED_WORDS, SENTINEL))
            red2 = _twice(dev, lambda: L.pa_k_hist_gram_owned(m, K, q, d_ring, ldh, head, cap, None, 0, d_dl, d_panel, ts,
                                                              dev.part, d_red2, off_do, 0), d_red2, RED_WORDS)
            assert red2[off_do:off_do + K * q].tobytes() == red[off_do:off_do + K * q].tobytes()
            assert (_outside(red2, [(off_do, K * q)]) == SENTINEL).all(), (K, q)

            # ---- the combine: x0[src[r]] = (Xl c)(r), the bits of pa_k_hist_combine; other rows keep the sentinel ----
            c = rng.standard_normal((K, q))
            d_c = dev.up(np.ascontiguousarray(c.T))
            d_x0 = dev.up(np.full((q, ldg), SENTINEL))
            x0 = _twice(dev, lambda: L.pa_k_hist_combine_owned(m, N, K, q, d_ring, ldh, head, cap, d_c, d_src, d_x0, ldg),
                        d_x0, q * ldg).reshape(q, ldg)
            others = np.ones(ldg, dtype=bool)
            others[src] = False
            assert (x0[:, others] == SENTINEL).all(), (K, q)
            assert (np.abs(x0[:, src].T - H.combine_exact(X, c)) <= H.combine_bound(X, c)).all(), (K, q)
            spread = np.zeros((N, cap))
            spread[src] = np.where(np.isnan(ring), 0.0, ring)
            d_spread, d_ref = dev.up(_colmajor(spread, ldg)), dev.up(np.full((q, ldg), SENTINEL))
            assert L.pa_k_hist_combine(N, K, q, d_spread, ldg, head, cap, d_c, d_ref, ldg) == 0, L.pa_rt_error()
            ref = dev.down(d_ref, q * ldg).reshape(q, ldg)
            assert x0[:, src].tobytes() == ref[:, src].tobytes(), (K, q)

            # ---- the gather: exact, each column to a slot of its own, a negative slot skipped ----
            A = rng.standard_normal((m, q))
            d_a = dev.up(_global(A, src, N, ldg))
            slots = rng.permutation(16)[:q].astype(np.int32)
            if q > 1:
                slots[q // 2] = -1
            d_out = dev.up(np.full((16, ldh), SENTINEL))
            out = _twice(dev, lambda: L.pa_k_hist_gather(m, N, q, d_src, d_a, ldg, slots.ctypes.data, 16, d_out, ldh), d_out,
                         16 * ldh).reshape(16, ldh)
            want = np.full((16, ldh), SENTINEL)
            for j in range(q):
                if slots[j] >= 0:
                    want[slots[j], :m] = A[:, j]
            assert out.tobytes() == want.tobytes(), (K, q)
            # no slots given: column j to column j (the staging of the owned rows)
            d_out = dev.up(np.full((q, ldh), SENTINEL))
            assert L.pa_k_hist_gather(m, N, q, d_src, d_a, ldg, None, q, d_out, ldh) == 0, L.pa_rt_error()
            out = dev.down(d_out, q * ldh).reshape(q, ldh)
            assert out[:, :m].tobytes() == np.ascontiguousarray(A.T).tobytes() and (out[:, m:] == SENTINEL).all()

            # ---- the ring in the operator's units: a true division, by physical slot ----
            live = np.where(np.isnan(ring[:, :K]), 1.0, ring[:, :K])
            d_live, d_sc = dev.up(_colmajor(live, ldh)), dev.up(np.full((K, m), SENTINEL))
            assert L.pa_k_hist_ring_scaled(m, K, d_live, ldh, d_dl, d_sc, m) == 0, L.pa_rt_error()
            assert dev.down(d_sc, K * m).tobytes() == np.ascontiguousarray((live / dl[:, None]).T).tobytes()
            dev.free_all_but_part()


def test_an_empty_ring_still_sums_the_right_hand_sides(dev):
    """K = 0: the projection's launch forms the b_j^2 words alone, and the combine writes zeros at the owned rows."""
    L = dev.L
    rng = np.random.default_rng(7)
    m, N, q = 300, 337, 3
    src = rng.permutation(N)[:m].astype(np.int32)
    Bo = rng.standard_normal((m, q))
    d_src, d_b = dev.up(src), dev.up(_global(Bo, src, N, N))
    d_red = dev.up(np.full(RED_WORDS, SENTINEL))
    assert L.pa_k_hist_project_owned(m, N, 0, q, None, 1, 0, 1, d_src, d_b, N, dev.part, d_red, 1, 1 + q) == 0, L.pa_rt_error()
    red = dev.down(d_red, RED_WORDS)
    exact = (Bo.astype(LD) ** 2).sum(axis=0)
    assert (np.abs(red[1:1 + q] - exact) <= H.gamma(m) * exact).all()
    assert (_outside(red, [(1, q)]) == SENTINEL).all()
    d_x0 = dev.up(np.full((q, N), SENTINEL))
    assert L.pa_k_hist_combine_owned(m, N, 0, q, None, 1, 0, 1, None, d_src, d_x0, N) == 0, L.pa_rt_error()
    x0 = dev.down(d_x0, q * N).reshape(q, N)
    others = np.ones(N, dtype=bool)
    others[src] = False
    assert not x0[:, src].any() and (x0[:, others] == SENTINEL).all()
    dev.free_all_but_part()


def test_the_owned_launchers_refuse_what_does_not_fit(dev):
    L = dev.L
    d = dev.up(np.ones(64 * 16))
    d_i = dev.up(np.zeros(64, dtype=np.int32))
    d_red = dev.up(np.zeros(RED_WORDS))
    cap = 16
    for K, q in ((-1, 1), (17, 1), (1, 0), (1, 17)):
        assert L.pa_k_hist_project_owned(8, 8, K, q, d, 8, 0, cap, d_i, d, 8, dev.part, d_red, 1, 17) != 0
        assert "pa_k_hist_project_owned" in L.pa_rt_error().decode()
        assert L.pa_k_hist_gram_owned(8, K, q, d, 8, 0, cap, d, 8, d, d, 16, dev.part, d_red, 1, 257) != 0
        assert "pa_k_hist_gram_owned" in L.pa_rt_error().decode()
    for K, q in ((-1, 1), (17, 1), (1, 0), (1, 17)):
        assert L.pa_k_hist_combine_owned(8, 8, K, q, d, 8, 0, cap, d, d_i, d, 8) != 0
        assert "pa_k_hist_combine_owned" in L.pa_rt_error().decode()
    for q in (0, 17):
        assert L.pa_k_hist_gather(8, 8, q, d_i, d, 8, None, 16, d, 8) != 0
        assert "pa_k_hist_gather" in L.pa_rt_error().decode()
    for K in (0, 17):
        assert L.pa_k_hist_ring_scaled(8, K, d, 8, d, d, 8) != 0
        assert "pa_k_hist_ring_scaled" in L.pa_rt_error().decode()
    assert L.pa_k_hist_project_owned(8, 8, 4, 2, d, 7, 0, 4, d_i, d, 8, dev.part, d_red, 1, 3) != 0      # ldh below the rows
    assert L.pa_k_hist_project_owned(8, 8, 4, 2, d, 8, 4, 4, d_i, d, 8, dev.part, d_red, 1, 3) != 0      # head outside the ring
    assert L.pa_k_hist_project_owned(8, 8, 4, 2, d, 8, 0, 3, d_i, d, 8, dev.part, d_red, 1, 3) != 0      # a ring smaller than K
    assert L.pa_k_hist_project_owned(8, 9, 4, 2, d, 8, 0, 4, d_i, d, 8, dev.part, d_red, 1, 3) != 0      # ldb below the N rows
    assert L.pa_k_hist_project_owned(8, 8, 4, 2, d, 8, 0, 4, d_i, d, 8, dev.part, d_red, 0, 3) != 0      # a block on word 0
    assert L.pa_k_hist_project_owned(8, 8, 4, 2, d, 8, 0, 4, d_i, d, 8, dev.part, d_red, 1, 2) != 0      # blocks that overlap
    assert L.pa_k_hist_project_owned(8, 8, 4, 2, d, 8, 0, 4, d_i, d, 8, dev.part, d_red, 1, RED_WORDS - 7) != 0   # past the end
    assert L.pa_k_hist_gram_owned(8, 2, 4, d, 8, 0, 2, d, 8, d, d, 2, dev.part, d_red, 1, 9) != 0        # a panel narrower than q
    assert L.pa_k_hist_gram_owned(8, 2, 4, d, 8, 0, 2, d, 7, d, d, 4, dev.part, d_red, 1, 9) != 0        # ldn below the rows
    assert L.pa_k_hist_gram_owned(8, 0, 4, None, 8, 0, 1, None, 0, d, d, 4, dev.part, d_red, 1, 1) != 0  # nothing on the left
    slots = np.array([0, 16], dtype=np.int32)
    assert L.pa_k_hist_gather(8, 8, 2, d_i, d, 8, slots.ctypes.data, 16, d, 8) != 0                      # a slot outside the ring
    assert L.pa_k_hist_gather(8, 9, 2, d_i, d, 8, None, 16, d, 8) != 0                                    # lda below the N rows
    assert L.pa_k_hist_combine_owned(8, 8, 2, 2, d, 8, 0, 2, d, d_i, d, 7) != 0                           # ldx0 below the N rows
    dev.L.preAlps_hip_sync()
