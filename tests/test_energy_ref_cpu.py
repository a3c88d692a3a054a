"""The NumPy restatement of the energy-norm drops (tests/energy_ref.py) against a dense solve, without a GPU: the
identity e_i^2 - e_{i+1}^2 = delta(i) that the device kernel's output is later measured by, and the window rule of the
library's host unit (through ctypes, in plan-only mode) with its defaults tau = 0.1, dmin = 4 on Poisson 10^3 in 40
parts and on elasticity 12 x 10 x 10 in 150 boxes.

Seen here (Orthodir and Orthomin agree to the digits shown):
  identity defect / e_0^2:  Poisson 7e-16 .. 2e-15, elasticity 2e-13 .. 8e-13 (the dense solve's own error, below)
  smallest est / true while the true error is above 1e-7 e_0:
    Poisson     (k, s) = (1, 4) 0.9954, (2, 2) 0.9913, (4, 1) 0.9934, (2, 4) 0.9947; warm (2, 2) 0.9964, (2, 4) 0.9974
    elasticity  (1, 4) 0.9705, (2, 2) 0.9705, (4, 1) 0.9509, (2, 4) 0.9706
  so the stop tests on the device use the Poisson inputs only (energy_ref.STOP_INPUTS): sqrt(0.95) = 0.9747.
  The stop at tol = 1e-5 comes 20 .. 24 iterations in on Poisson and 37 .. 51 on elasticity, where the true relative
  energy error is 3e-8 .. 8e-7: the delay of the lower bound makes the test conservative."""
import numpy as np
import pytest

import energy_ref as R

CONFIGS = [(1, 4), (2, 2), (4, 1), (2, 4)]      # t = 4 with k in {1, 2, 4}, t = 8 with k = 2
# The true errors come from a dense LU solve: x* carries a relative error of about cond(A0) eps, and e^T A0 e of a small e
# inherits it relative to e_0^2 once e itself is at that level.  cond(A0) is below 1e5 for both matrices (Poisson 10^3:
# about 50; the elasticity block: a few 1e4), so 1e5 * 2^-52 = 2.2e-11 bounds what the reference can resolve.
IDENTITY_BOUND = 1e5 * 2.0 ** -52

_pbs = {}


def _pb(name):
    if name not in _pbs:
        for other in list(_pbs):
            _pbs.pop(other)["prob"].close()
        _pbs[name] = R.open_problem(name, plan_only=True)
    return _pbs[name]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for name in list(_pbs):
        _pbs.pop(name)["prob"].close()


def _defect(r):
    d, e2 = r["delta"], r["e2"]
    return (np.abs(e2[:-1] - e2[1:] - d).max(axis=0) / e2[0]).max()


@pytest.mark.parametrize("alg", ["odir", "omin"])
@pytest.mark.parametrize("k,s", CONFIGS)
@pytest.mark.parametrize("name", ["P", "E"])
def test_one_iteration_takes_delta_off_the_squared_energy_error(name, k, s, alg):
    pb = _pb(name)
    r = R.restated(pb, k, s, alg)
    d, e2 = r["delta"], r["e2"]
    assert d.shape == (len(e2) - 1, k) and (d >= 0.0).all()
    defect = _defect(r)
    print(name, k, s, alg, "iterations", len(d), "defect / e_0^2", defect)
    assert defect <= IDENTITY_BOUND
    # telescoped: what the device test checks with the library's drops
    assert (np.abs(d.sum(axis=0) - (e2[0] - e2[-1])) <= IDENTITY_BOUND * e2[0]).all()
    assert (e2[-1] <= 1e-20 * e2[0]).all()                 # (the run went down to the floor it was given)


@pytest.mark.parametrize("name,k,s,warm", R.STOP_INPUTS)
def test_the_stop_inputs_keep_the_estimate_within_five_percent(name, k, s, warm):
    """est^2 / true^2 >= 0.95 while the true error is above 1e-7 e_0, and the estimate never exceeds the truth; the stop
    at tol = 1e-5 exists and leaves a true error under tol * e_0.  With a guess e_0 is the guess's error."""
    pb = _pb(name)
    X0 = R.guess(pb, k, s) if warm else None
    r = R.restated(pb, k, s, "odir", X0, key=warm)
    assert _defect(r) <= IDENTITY_BOUND
    worst, seen = R.worst_ratio(r["delta"], r["e2"])
    n, windows = R.stop_iteration(r["delta"], 1e-5)
    print(name, k, s, warm, "smallest est / true", worst, "over", seen, "windows; stop at", n, "true error / e_0",
          np.sqrt(r["e2"][n] / r["e2"][0]))
    assert seen >= 10 and np.sqrt(0.95) <= worst <= 1.0 + 1e-9
    assert n is not None and R.DMIN < n < len(r["delta"])
    assert (r["e2"][n] <= 1e-10 * r["e2"][0]).all()
    for j, (l, est2) in enumerate(windows):
        assert 0 <= l <= n - R.DMIN and est2 <= 1e-10 * r["delta"][:n, j].sum() * (1 + 1e-12)


@pytest.mark.parametrize("k,s", CONFIGS)
def test_elasticity_is_a_lower_bound_but_not_within_five_percent(k, s):
    """Recorded, and the reason no stop test on the device leans on this problem: the estimate stays a lower bound, but
    its smallest ratio is 0.951 .. 0.971 (module docstring)."""
    pb = _pb("E")
    r = R.restated(pb, k, s, "odir")
    worst, seen = R.worst_ratio(r["delta"], r["e2"])
    print("E", k, s, "smallest est / true", worst, "over", seen, "windows")
    assert seen >= 10 and 0.9 <= worst <= 1.0 + 1e-9


def test_the_python_view_of_the_tracker_matches_its_layout():
    """energy_ref.HostUnit mirrors pa_energy_t by hand: a field out of place shows as a wrong count or window."""
    u = R.HostUnit(2, 40)
    try:
        for i in range(30):
            assert u.push(np.array([0.5 ** i, 1.0])) == 0
        assert (u.e.k, u.e.cap, u.e.n, u.e.tau, u.e.dmin, u.e.nan) == (2, 40, 30, R.TAU, R.DMIN, 0)
        l = u.window(0)
        assert l == u.e.window[0] == u.e.last[0] and 15 <= l <= 26 and u.window(1) == -1 and u.e.last[1] == -1
        want = sum(0.5 ** i for i in range(29, l - 1, -1))
        assert u.sum(0, l) == want == u.e.suffix[l] and u.e.delta[40 + 7] == 1.0
        assert u.goes_on(1e-5)                              # (system 1 has no window)
    finally:
        u.close()
