"""Device plumbing of the kernel tests that call the pa_k_* launchers through ctypes (test_gpu_row_pass.py,
test_gpu_gram_finish.py, test_gpu_dense_kernels.py): buffers through pa_rt_malloc / _memset / _h2d / _d2h / _free,
every one zeroed when it is made and freed by close().  Small blocks travel column-major.

Not a test module: nothing here is collected."""
import ctypes as C

import numpy as np

vp, ci = C.c_void_p, C.c_int
pi = C.POINTER(C.c_int)

SIGNATURES = {
    "pa_k_update_xrz_mode": [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, pi, vp, vp, ci, vp, ci, vp],
    "pa_k_flush_x": [ci, ci, ci, vp, vp, vp, vp],
    "pa_k_trace_finish": [vp, ci, ci, ci, vp, vp, vp],
    "pa_k_finish32": [vp, ci, vp, ci, ci, vp, vp, vp, vp],
    "pa_k_finish32_pair": [vp, ci, vp, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp],
    "pa_k_finish32_trace": [vp, ci, vp, vp, vp, ci, ci, ci, vp, vp],
    "pa_k_potrf_alpha": [vp, ci, ci, vp, vp, vp],
    "pa_k_gram_finish": [ci, ci, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, ci, vp, vp, vp],
    "pa_k_gram_finish_trace": [ci, ci, vp, vp, vp, vp, ci, ci, ci, vp, ci, vp, ci, ci, vp, vp],
    "pa_k_finish": [vp, ci, ci, ci, ci, ci, ci, vp, ci],
    "pa_k_trsm_update": [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, pi, ci, vp, vp, vp, vp, vp],
    "pa_k_update_z": [ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, pi],
    "pa_k_update_z_pack": [ci, vp, vp, vp],
}


class Dev:
    def __init__(self):
        import prealps_amd
        from prealps_amd.lib import check
        self.L, self.check = prealps_amd.load(), check
        L = self.L
        check(L.preAlps_hip_init(0), "init")
        L.pa_rt_error.restype = C.c_char_p
        L.pa_rt_malloc.restype = vp
        L.pa_rt_malloc.argtypes = [C.c_size_t]
        L.pa_rt_free.argtypes = [vp]
        L.pa_rt_free.restype = None
        L.pa_rt_memset.argtypes = [vp, ci, C.c_size_t]
        L.pa_rt_h2d.argtypes = [vp, vp, C.c_size_t]
        L.pa_rt_d2h.argtypes = [vp, vp, C.c_size_t]
        for name, args in SIGNATURES.items():
            f = getattr(L, name)
            f.argtypes, f.restype = args, ci
        self.bufs = []

    def zeros(self, nbytes):
        nbytes = max(int(nbytes), 8)
        d = self.L.pa_rt_malloc(nbytes)
        assert d
        self.bufs.append(d)
        self.check(self.L.pa_rt_memset(d, 0, nbytes), "memset")
        return d

    def put(self, d, a):
        """A host array as it lies in memory -> the device buffer d."""
        a = np.ascontiguousarray(a)
        self.check(self.L.pa_rt_h2d(d, a.ctypes.data, a.nbytes), "h2d")

    def up(self, a, extra=0):
        """A new device buffer holding a (C order: a panel, a stack of blocks) and `extra` zero bytes behind it."""
        a = np.ascontiguousarray(a)
        d = self.zeros(a.nbytes + extra)
        if a.nbytes:
            self.put(d, a)
        return d

    def upf(self, a, ld=None):
        """A small block, column-major with leading dimension ld (the padding rows are zero)."""
        a = np.asarray(a, dtype=np.float64)
        ld = a.shape[0] if ld is None else ld
        h = np.zeros((a.shape[1], ld))
        h[:, :a.shape[0]] = a.T
        return self.up(h)

    def down(self, d, shape, dtype=np.float64):
        """The device buffer as a C-order array of this shape."""
        h = np.zeros(shape, dtype=dtype)
        self.sync()
        self.check(self.L.pa_rt_d2h(h.ctypes.data, d, h.nbytes), "d2h")
        return h

    def downf(self, d, rows, cols, ld=None):
        """A column-major block of leading dimension ld as a (rows, cols) array."""
        ld = rows if ld is None else ld
        return self.down(d, (cols, ld))[:, :rows].T.copy()

    def sync(self):
        self.check(self.L.preAlps_hip_sync(), "sync")

    def error(self):
        return self.L.pa_rt_error().decode()

    def close(self):
        for d in self.bufs:
            self.L.pa_rt_free(d)
        self.bufs = []
