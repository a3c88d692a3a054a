"""pa_k_energy_drops alone (prealps_amd/csrc/dense_energy.hip): the energy-norm drops delta_j = sum_r (sum_{c in G_j}
alpha(r, c))^2 of a random alpha, through ctypes on raw device buffers and pinned host words, against long double.

The bound (the way of DESIGN section 4o: every floating-point sum against the sum of its absolute terms): v_r is formed
by s - 1 <= T additions and squared, then `rows` fused multiply-adds add the squares up, so with u = 2^-53
    |computed - exact| <= (2 T + rows + 2) u * sum_r (sum_{c in G_j} |alpha(r, c)|)^2.
The padding rows of alpha (ld > rows) and the columns behind the last system hold NaN: a read out of place shows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
vp, ci = C.c_void_p, C.c_int


class Dev:
    """Raw buffers for this kernel: device memory through pa_rt_malloc, and the pinned words the host reads."""

    def __init__(self):
        import prealps_amd
        from prealps_amd.lib import check
        self.L, self.check = prealps_amd.load(), check
        L = self.L
        check(L.preAlps_hip_init(0), "init")
        L.pa_rt_error.restype = C.c_char_p
        for name in ("pa_rt_malloc", "pa_rt_host_alloc_coherent"):
            getattr(L, name).restype = vp
            getattr(L, name).argtypes = [C.c_size_t]
        for name in ("pa_rt_free", "pa_rt_host_free"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [vp]
        L.pa_rt_memset.argtypes = [vp, ci, C.c_size_t]
        L.pa_rt_h2d.argtypes = [vp, vp, C.c_size_t]
        L.pa_rt_d2h.argtypes = [vp, vp, C.c_size_t]
        L.pa_k_energy_drops.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp]
        L.pa_k_energy_drops.restype = ci
        self.bufs, self.pinned = [], []

    def up(self, a):
        a = np.ascontiguousarray(a)
        d = self.L.pa_rt_malloc(max(a.nbytes, 8))
        assert d
        self.bufs.append(d)
        self.check(self.L.pa_rt_h2d(d, a.ctypes.data, a.nbytes), "h2d")
        return d

    def down(self, d, n):
        h = np.zeros(n)
        self.check(self.L.preAlps_hip_sync(), "sync")
        self.check(self.L.pa_rt_d2h(h.ctypes.data, d, h.nbytes), "d2h")
        return h

    def host_words(self, n, fill):
        p = self.L.pa_rt_host_alloc_coherent(n * 8)
        assert p
        self.pinned.append(p)
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(n,))
        a[:] = fill
        return p, a

    def drops(self, alpha, rows, ld, T, k, s, out, host):
        return self.L.pa_k_energy_drops(alpha, rows, ld, T, k, s, out, host)

    def error(self):
        return self.L.pa_rt_error().decode()

    def close(self):
        self.L.preAlps_hip_sync()
        for d in self.bufs:
            self.L.pa_rt_free(d)
        for p in self.pinned:
            self.L.pa_rt_host_free(p)
        self.bufs, self.pinned = [], []


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def _cases():
    out = []
    for T in (1, 2, 4, 8, 16):
        ks = sorted({1, T} | ({2} if T in (4, 8) else {4} if T == 16 else set()))
        for k in ks:
            out.append((T, T, T + 3, k, T // k))           # ld > rows
    out += [(16, 16, 16, 1, 16), (4, 4, 4, 2, 2),           # ld = rows, as the iteration passes it
            (3, 8, 5, 3, 2), (1, 16, 2, 5, 3), (16, 2, 16, 1, 1)]      # rows != T, columns left over behind the systems
    return out


@pytest.mark.parametrize("rows,T,ld,k,s", _cases())
def test_the_drops_against_long_double(dev, rows, T, ld, k, s):
    rng = np.random.default_rng(1000 * T + 10 * k + rows)
    a = rng.standard_normal((rows, T)) * 10.0 ** rng.uniform(-3, 3, size=(rows, T))      # six decades within a sum
    h = np.full((T, ld), np.nan)
    h[:k * s, :rows] = a[:, :k * s].T                                                # column major; NaN wherever nothing may be read
    d_alpha = dev.up(h)
    d_out = dev.up(np.full(16, -7.0))
    p_host, host = dev.host_words(16, -7.0)
    assert dev.drops(d_alpha, rows, ld, T, k, s, d_out, p_host) == 0, dev.error()
    got = dev.down(d_out, 16)
    al = a.astype(np.longdouble)
    for j in range(k):
        grp = al[:, j * s:(j + 1) * s]
        want = (grp.sum(axis=1) ** 2).sum()
        bound = (2 * T + rows + 2) * U53 * float((np.abs(grp).sum(axis=1) ** 2).sum())
        print("T", T, "k", k, "system", j, "error", float(abs(got[j] - want)), "bound", bound)
        assert abs(np.longdouble(got[j]) - want) <= bound
    assert (got[k:] == -7.0).all()                                   # nothing behind the k values is written
    assert host.tobytes() == got.tobytes()                            # the pinned words are the device slot, bit for bit
    # a second launch, and one without the host words: the same bits
    d_out2 = dev.up(np.full(16, -7.0))
    assert dev.drops(d_alpha, rows, ld, T, k, s, d_out2, None) == 0, dev.error()
    assert dev.down(d_out2, 16).tobytes() == got.tobytes()


def test_refusals(dev):
    d_alpha = dev.up(np.ones((16, 16)))
    d_out = dev.up(np.full(16, -7.0))
    good = dict(alpha=d_alpha, rows=4, ld=4, T=4, k=2, s=2, out=d_out, host=None)
    for change, word in [(dict(alpha=None), "no alpha"), (dict(out=None), "no place"), (dict(rows=0), "0 x 4"),
                         (dict(rows=17, ld=17), "17 x 4"), (dict(T=0), "4 x 0"), (dict(T=17), "4 x 17"),
                         (dict(ld=3), "leading dimension 3"), (dict(k=0), "0 systems"), (dict(s=0), "of 0 columns"),
                         (dict(k=3), "3 systems of 2 columns do not fit the 4 columns"), (dict(k=-1), "-1 systems")]:
        a = dict(good, **change)
        rc = dev.drops(a["alpha"], a["rows"], a["ld"], a["T"], a["k"], a["s"], a["out"], a["host"])
        assert rc != 0, change
        assert "pa_k_energy_drops" in dev.error() and word in dev.error(), (change, dev.error())
    assert (dev.down(d_out, 16) == -7.0).all()                        # a refusal launches nothing
    assert dev.drops(good["alpha"], 4, 4, 4, 2, 2, d_out, None) == 0
    assert (dev.down(d_out, 2) == 16.0).all()                         # four rows of (1 + 1)^2
