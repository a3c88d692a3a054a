"""The kernel units report through the runtime's error channel: a pa_k_* launcher that refuses its arguments
returns 1 and leaves its reason where pa_rt_error() finds it -- and so every PA_CHECK and PA_FAIL of the host
code, whose text preAlps_hip_last_error() hands on.  The launchers here refuse before any HIP call (no
stream is looked up, nothing is launched), so the checks need no GPU."""
import ctypes as C

import pytest

import prealps_amd


@pytest.fixture(scope="module")
def L():
    lib = prealps_amd.load()
    lib.pa_rt_error.restype = C.c_char_p
    return lib


def _refused(L, rc, reason):
    assert rc == 1
    assert reason in L.pa_rt_error().decode()


def test_multi_start_reports_systems_that_do_not_fit(L):
    nblk = C.c_int(-1)
    rc = L.pa_k_multi_start(64, 4, 3, 2, None, 64, None, None, None, C.byref(nblk))
    _refused(L, rc, "pa_k_multi_start: 3 systems of 2 columns do not fit a panel of stride 4")
    assert nblk.value == -1


def test_update_xrz_reports_the_panel_width(L):
    nblk = C.c_int(-1)
    rc = L.pa_k_update_xrz(64, 8, 4, None, None, None, None, None, None, None, None, None, C.byref(nblk),
                           None, None, 8, None)
    _refused(L, rc, "pa_k_update_xrz: 4-column panels with lazy normalisation only")
    assert nblk.value == -1


def test_block_solve_reports_what_its_planner_refuses(L):
    """bj_g4.hip reports where the other kernel units do: a plan of all zeros has records of 0 bits, which the launch
    planner (bj_g4_plan.c) refuses before anything is looked up or launched"""
    plan = C.create_string_buffer(1024)            # a zero-filled pa_bj_plan_t (and room to spare)
    L.pa_k_bj_g4.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                             C.c_void_p]
    L.pa_k_bj_g4.restype = C.c_int
    rc = L.pa_k_bj_g4(plan, None, 1, 8, 64, 4, 4, None, None, None)
    _refused(L, rc, "pa_k_bj_g4: records of 0 bits (64 or 32)")


class _BjPlan(C.Structure):
    """pa_bj_plan_t (pa_device.h)"""
    _fields_ = ([("nparts", C.c_int)] +
                [(n, C.c_void_p) for n in ("row0", "nrows", "bw", "off", "map_f", "map_b", "Lf", "Lb", "Lf2", "Lb2", "off2", "Lg4")] +
                [("g4_bits", C.c_int)] + [(n, C.c_void_p) for n in ("class_g4", "class_bmax", "invd_f", "invd_b")] +
                [("nclass", C.c_int), ("class_R", C.POINTER(C.c_int)), ("class_count", C.POINTER(C.c_int)),
                 ("class_wmax", C.POINTER(C.c_int)), ("class_list", C.POINTER(C.c_void_p)), ("class_ptask", C.c_void_p),
                 ("pair_mode", C.c_int), ("pair_intact", C.c_int)])


def test_band_solve_reports_a_stride_its_wide_kernels_do_not_have(L):
    """pa_k_bj_apply on a plan with one wide class and a panel stride of 3: the dispatch planner (bj_band_plan.c)
    refuses, for wide classes as for narrow ones, before anything is launched"""
    one = lambda v: (C.c_int * 1)(v)
    plan = _BjPlan(nclass=1, class_R=one(-1), class_count=one(5), class_wmax=one(300), class_list=(C.c_void_p * 1)(None))
    L.pa_k_bj_apply.argtypes = [C.POINTER(_BjPlan), C.c_int, C.c_void_p, C.c_void_p]
    L.pa_k_bj_apply.restype = C.c_int
    rc = L.pa_k_bj_apply(C.byref(plan), 3, None, None)
    _refused(L, rc, "pa_k_bj_apply: unsupported panel stride 3")


def test_rowsum_reports_an_unsupported_stride(L):
    rc = L.pa_k_rowsum(64, 3, 3, None, None)
    _refused(L, rc, "unsupported panel stride 3")
