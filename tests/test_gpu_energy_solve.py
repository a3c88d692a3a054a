"""The energy-norm error estimate through the solver: preAlps_ECGSolveSystemEnergy / EcgProblem.solve_system(stop="energy",
energy=True) on the device against the NumPy restatement of tests/energy_ref.py and a dense solve of the caller's matrix.

Problems: P = Poisson 10^3 in 40 parts, E = elasticity 12 x 10 x 10 in 150 boxes; right-hand sides
default_rng(20260407).standard_normal((N, 16)) in the caller's space.  The stop tests use the Poisson inputs alone
(energy_ref.STOP_INPUTS: the reference keeps est / true >= sqrt(0.95) there, tests/test_energy_ref_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import energy_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
RTOL_HIST = 1e-8          # first-8 histories against another fp64 implementation

_open = {}


def _problem(name):
    if name in _open:
        return _open[name]
    for other in list(_open):
        _open.pop(other)["prob"].close()
    pb = R.open_problem(name, device=0)
    pb["prob"].create_block_jacobi()
    _open[name] = pb
    return pb


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for name in list(_open):
        _open.pop(name)["prob"].close()


class _switches:
    """PREALPS_ECG_SOLVE_FIRST / PREALPS_ECG_X_DEFER for the solves inside (both are read at every start)."""

    def __init__(self, solve_first, x_defer):
        self.want = {"PREALPS_ECG_SOLVE_FIRST": str(solve_first), "PREALPS_ECG_X_DEFER": str(x_defer)}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.want}
        os.environ.update(self.want)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


VARIANTS = {"first-defer": ("odir", 1, 1), "first-every": ("odir", 1, 0), "plain": ("odir", 0, 1), "omin": ("omin", 1, 1)}


def _alg(alg):
    import prealps_amd as pa
    return pa.ORTHODIR if alg == "odir" else pa.ORTHOMIN


def _drop_cases():
    out = []
    for name in ("P", "E"):
        for k, s in [(1, 4), (2, 2), (4, 1)]:
            out += [(name, k, s, v) for v in VARIANTS]
        out += [(name, 2, 4, "plain"), (name, 2, 4, "omin")]          # t = 8: the order of solve_first_step does not apply
    return out


# ---- 1. the drops ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,s,variant", _drop_cases())
def test_the_drops_are_the_restatements_and_telescope(name, k, s, variant):
    """The first 8 rows of drop_hist agree with the restatement to 1e-8; sum_i delta_j(i) = e_0^2 - e_n^2 with both errors
    from a dense solve of the caller's unscaled, unpermuted matrix and the returned x, within 100 times the defect the CPU
    reference itself shows on the same case (seen: DESIGN section 4t)."""
    alg, sf, xd = VARIANTS[variant]
    pb = _problem(name)
    ref = R.restated(pb, k, s, alg)
    with _switches(sf, xd):
        got = pb["prob"].solve_system(pb["B"][:, :k], k * s, stop="scaled", tol=TOL, ortho_alg=_alg(alg), energy=True)
    n = got.iters
    assert n > 8 and got.drop_hist.shape == (n, k) and got.err_hist.shape == (n + 1, k)
    np.testing.assert_allclose(got.drop_hist[:8], ref["delta"][:8], rtol=RTOL_HIST, atol=0.0)
    xstar = R.exact(pb, k)
    e0, en = R.energy2(pb, xstar), R.energy2(pb, xstar - got.x)
    own = (np.abs(ref["e2"][:-1] - ref["e2"][1:] - ref["delta"]).max(axis=0) / ref["e2"][0]).max()
    defect = np.abs(got.drop_hist.sum(axis=0) - (e0 - en)) / e0
    print(name, k, s, variant, "iterations", n, "telescoping defect / e_0^2", defect, "the reference's own", own)
    assert (defect <= 100.0 * own).all()
    np.testing.assert_allclose(got.energy_norm, np.sqrt(got.drop_hist.sum(axis=0)), rtol=1e-13)
    # the estimates are lower bounds of the true errors of the restatement's iterates (same iterates to 1e-8)
    for j in range(k):
        L = got.err_iter[j]
        if L >= 0:
            assert got.err_est[j] == got.err_hist[L, j] > 0.0 and (got.err_hist[L + 1:, j] == -1.0).all()
            assert (got.err_hist[:L + 1, j] <= np.sqrt(ref["e2"][:L + 1, j]) * (1 + 1e-6)).all()
        else:
            assert got.err_est[j] == -1.0 and (got.err_hist[:, j] == -1.0).all()


# ---- 2. what exists is unchanged ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["first-defer", "plain", "omin"])
@pytest.mark.parametrize("stop", ["original", "scaled"])
@pytest.mark.parametrize("k,s,warm", [(1, 4, False), (2, 2, True)])
def test_tracking_changes_no_bit_and_costs_one_launch_per_iteration(k, s, warm, stop, variant):
    alg, sf, xd = VARIANTS[variant]
    pb = _problem("P")
    prob = pb["prob"]
    B = pb["B"][:, :k]
    X0 = R.guess(pb, k, s) if warm else None
    with _switches(sf, xd):
        c0 = prob.stat("ecg_energy_launches")
        base = prob.solve_system(B, k * s, x0=X0, stop=stop, tol=TOL, ortho_alg=_alg(alg))
        c1 = prob.stat("ecg_energy_launches")
        got = prob.solve_system(B, k * s, x0=X0, stop=stop, tol=TOL, ortho_alg=_alg(alg), energy=True)
        c2 = prob.stat("ecg_energy_launches")
    assert base.drop_hist is None and c1 == c0
    assert got.iters == base.iters > 0 and c2 - c1 == got.iters
    assert np.ascontiguousarray(got.x).tobytes() == np.ascontiguousarray(base.x).tobytes()
    for key in ("res", "bs", "sys_hist", "sys_normb", "sys_res", "sys_res_original"):
        assert getattr(got, key).tobytes() == getattr(base, key).tobytes(), key
    assert (got.final_res, got.normb, got.final_bs, got.metric) == (base.final_res, base.normb, base.final_bs, stop)
    assert got.drop_hist.shape == (got.iters, k) and (got.drop_hist > 0.0).all()


def test_without_its_flags_the_entry_is_solve_system():
    import prealps_amd as pa
    pb = _problem("P")
    prob, L, N, k, t = pb["prob"], pb["prob"].L, pb["N"], 2, 4
    want = prob.solve_system(pb["B"][:, :k], t, stop="scaled", tol=TOL)
    c0 = prob.stat("ecg_energy_launches")
    b = np.asfortranarray(pb["B"][:, :k])
    x = np.zeros((N, k), order="F")
    e = prob.new_ecg(t, pa.ORTHODIR, pa.NO_BS_RED, TOL, 1000)
    drops = np.full((1002, k), -5.0, order="F")
    nh = C.c_int()
    pd = C.POINTER(C.c_double)
    rc = L.preAlps_ECGSolveSystemEnergy(C.byref(e), k, b.ctypes.data, N, None, 0, x.ctypes.data, N, 0, float("nan"), -1,
                                        None, None, None, None, None, drops.ctypes.data_as(pd), None, None, None, None,
                                        1002, C.byref(nh))
    assert rc == 0, L.preAlps_hip_last_error()
    assert e.iter == want.iters == nh.value and x.tobytes() == np.asfortranarray(want.x).tobytes()
    assert (drops == -5.0).all() and prob.stat("ecg_energy_launches") == c0


# ---- 3. the stop test ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,s,warm", R.STOP_INPUTS)
def test_the_energy_stop_ends_where_the_host_unit_says(name, k, s, warm):
    """A run that the residual stops much later gives the drops; the host unit, fed them, names the iteration; the
    run with stop="energy" ends there, with those drops, and the true energy error of its x -- from the dense solve --
    is at most tol * ||x* - x0||_A."""
    pb = _problem(name)
    prob = pb["prob"]
    B = pb["B"][:, :k]
    X0 = R.guess(pb, k, s) if warm else None
    long_run = prob.solve_system(B, k * s, x0=X0, stop="scaled", tol=1e-11, max_iter=60, energy=True)
    n, windows = R.stop_iteration(long_run.drop_hist, TOL)
    assert n is not None and n < long_run.iters
    c0 = prob.stat("ecg_energy_launches")
    got = prob.solve_system(B, k * s, x0=X0, stop="energy", tol=TOL)
    assert got.iters == n and prob.stat("ecg_energy_launches") - c0 == n
    assert got.drop_hist.tobytes() == np.ascontiguousarray(long_run.drop_hist[:n]).tobytes()
    assert np.ascontiguousarray(got.x).tobytes() == np.ascontiguousarray(
        prob.solve_system(B, k * s, x0=X0, stop="scaled", tol=1e-11, max_iter=n).x).tobytes()
    for j, (l, est2) in enumerate(windows):
        assert got.err_iter[j] == l and got.err_est[j] == np.sqrt(est2)
        assert got.err_est[j] <= TOL * got.energy_norm[j]
    xstar = R.exact(pb, k)
    e0 = np.sqrt(R.energy2(pb, xstar - (X0 if warm else 0.0)))
    en = np.sqrt(R.energy2(pb, xstar - got.x))
    print(name, k, s, warm, "stop at", n, "true energy error / initial", en / e0, "estimate / initial", got.err_est / e0,
          "at iterations", got.err_iter)
    assert (en <= TOL * e0).all()
    assert (got.energy_norm <= e0 * (1 + 1e-12)).all()            # D_j(0, n) is a lower bound of the initial error


# ---- 4. refusals -------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry():
    import prealps_amd as pa
    from prealps_amd.lib import PreAlpsError
    pb = _problem("P")
    prob, N = pb["prob"], pb["N"]
    B = pb["B"][:, :2]
    c0 = prob.stat("ecg_energy_launches")
    for kw, word in [(dict(bs_red=pa.ADAPT_BS), "ADAPT_BS"), (dict(tau=0.0), "tau = 0"), (dict(tau=0.5), "tau = 0.5"),
                     (dict(tau=float("nan")), "tau = nan"), (dict(dmin=1), "dmin = 1"),
                     (dict(ortho_alg=pa.ORTHODIR_FUSED), "ORTHODIR_FUSED")]:
        for how in (dict(stop="energy"), dict(stop="scaled", energy=True)):
            with pytest.raises(PreAlpsError, match="preAlps_ECGSolveSystemEnergy") as err:
                prob.solve_system(B, 4, tol=TOL, **dict(kw, **how))
            assert word in str(err.value), str(err.value)
    with pytest.raises(ValueError):
        prob.solve_system(B, 4, stop="energy", refine=True)
    with pytest.raises(ValueError):
        prob.solve_system(B, 4, stop="energie")
    # both stopping tests at once, and an unknown bit: through the C entry
    L = prob.L
    b = np.asfortranarray(B)
    x = np.zeros((N, 2), order="F")
    nh = C.c_int()
    for flags, word in [(2 | 8, "two stopping tests"), (4 | 16, "unknown bits"), (8 | 32, "unknown bits")]:
        e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, TOL, 100)
        rc = L.preAlps_ECGSolveSystemEnergy(C.byref(e), 2, b.ctypes.data, N, None, 0, x.ctypes.data, N, flags, 0.1, 4,
                                            None, None, None, None, None, None, None, None, None, None, 0, C.byref(nh))
        msg = L.preAlps_hip_last_error().decode()
        assert rc != 0 and "preAlps_ECGSolveSystemEnergy" in msg and word in msg, msg
    e = prob.new_ecg(4, pa.ORTHODIR, pa.NO_BS_RED, TOL, 100)      # what preAlps_ECGSolveSystem refuses, under this entry's name
    rc = L.preAlps_ECGSolveSystemEnergy(C.byref(e), 0, b.ctypes.data, N, None, 0, x.ctypes.data, N, 4, 0.1, 4,
                                        None, None, None, None, None, None, None, None, None, None, 0, C.byref(nh))
    msg = L.preAlps_hip_last_error().decode()
    assert rc != 0 and "preAlps_ECGSolveSystemEnergy" in msg and "nrhs = 0" in msg, msg
    assert prob.stat("ecg_energy_launches") == c0 and (x == 0.0).all()
    # and the solver works afterwards
    assert prob.solve_system(B, 4, stop="energy", tol=TOL).iters > 0
