"""The block product A P on the block shapes a full device gets, checked element by element against a row-wise
error bound.

Inputs.  block_rows() of spmm_plan.c gives a workgroup one 64-row slice until the device has four workgroups per
compute unit: on 256 CUs two slices from 131 072 rows, three from 196 608, four from 262 144.  The cases of
spmm_block_cases.py (gen.node_graph_csr: three dofs per node, 17 .. 33 nonzeros per row) sit at those row counts, so
that wavefronts 1 .. 3 of spmm_runs_block and spmm_body work, blocks are halved to fit the staging area (4 -> 2 -> 1
slices in one launch), the staging area is at its cap, the run plan stages more than 64 KiB at 8 and 16 columns (the
hipFuncSetAttribute branch of launch_spmm) in two batches, slices of fewer than 64 rows sit inside blocks that span
subdomains, and the window kernel has blocks of several slices.  One operator per (case, switch setting); the
panel strides 2, 4, 8, 16 rebuild its plan in place.  After every product the statistics of the plan that ran are
held against spmm_block_cases.GEOMETRY (test_spmm_blocks_cpu.py holds the plan builder against the same table): a
device whose CU count cuts other plans fails there, with a message that says so.

Criterion.  (rp, ci, v) = prob.local_csr() has the pattern of the oracle's B and its values within 1e-15 relative.
With Yref = B_v X formed in np.longdouble, for every row i and column c

    |Y - Yref|[i, c] <= (nnz_i + 2) * 2^-53 * (|B_v| |X|)[i, c].

An fma chain over the nnz_i stored terms of a row commits nnz_i roundings in any order, each at most 2^-53 of a partial
sum that |B_v| |X| bounds (to first order; the two spare units cover the second order and the reference's own 2^-64),
and the padding terms of a plan are exact zeros: the bound is derived, not measured, and does not depend on the plan.
scipy's double-precision product sits at about 0.3 of it; one entry of one row read from the neighbouring staged row
sits 1e13 above it.  Every product is also finite and three more have the same bits.  Lines "BLOCKS ..." print per
case, stride and switch setting the asserted geometry and the kernel's worst ratio to the bound beside scipy's.

The Gram by-product.  spmm_gram_tail adds the shares of four wavefronts; with one-slice blocks three of them are
zero.  base4's pattern with excess 0.02 (Orthodir t = 4 needs more than 15 iterations at tol 1e-5) is solved under
the three plans that leave the block behind -- k_spmm_runs_gram<1> (default, staged), <3> (PREALPS_SPMM_RUNS=2) and
k_spmm_gram (PREALPS_SPMM_STAGED=0, blocks of 2 and 4 slices) -- against the oracle's iteration count and history, and
again with PREALPS_SPMM_GRAM=0 (read at every solve: _preAlps_ECGMalloc -> pa_operator_gram_blocks).  A 60-row
pentadiagonal matrix in 4 parts stages 19 to 21 rows, at most 672 bytes: less than the 1024 bytes the tail passes the shares
through, which the launcher has to request itself.

Measured on an MI355X: the 25 tests take 22 s together.  The first operator of a case forms the host references
(far3 3.3 s, base4 with its seven column counts 2.9 s, far2 2.0 s, ragged 1.5 s, three 1.1 s, two 0.7 s); every later
setting of the case takes 0.2 .. 1.1 s, a Gram solve pair 0.04 .. 0.4 s.  Worst ratios to the limit: kernel 0.25 ..
0.33, scipy 0.26 .. 0.40; the Gram histories follow the oracle's within 4e-13.
"""
import functools
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import spmm_block_cases as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RTOL_HIST = 1e-8            # (test_gpu_configs.py / test_gpu_parity.py)
PLAN_STATS = ("spmm_runs", "spmm_staged", "spmm_slices", "spmm_blocks", "spmm_stage_rows")


def _set_switches(monkeypatch, switch):
    env = dict(S.switch_env(switch), PREALPS_SPMM_GRAM=None)
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _cu_note():
    try:
        import torch
        return "this device has %d compute units, the table is cut for %d" % (
            torch.cuda.get_device_properties(0).multi_processor_count, S.CUS)
    except Exception as e:      # the note is a courtesy of the failure message
        return "the table is cut for %d compute units (this device's count is unknown: %s)" % (S.CUS, e)


class _Host:
    """What the host knows of a case: the oracle's scaled and permuted B, and per t the panel X, Yref in extended
    precision, the row-wise limit and scipy's own worst ratio.  Built once per case and left unchanged."""

    def __init__(self, case, excess=1.0):
        from oracle import oracle as O
        self.case = case
        self.rp, self.ci, self.v = S.matrix(case, excess)
        self.part, self.P, self.rowpos = S.partition(case)
        self.N = len(self.rp) - 1
        A = sp.csr_matrix((self.v, self.ci, self.rp), shape=(self.N, self.N))
        self.B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), self.part, self.P)
        assert np.array_equal(perm, np.arange(self.N)) and np.array_equal(rowpos, self.rowpos)
        self.values = None
        self.refs = {}

    def bind(self, rp, ci, v):
        """The library's panel: the oracle's pattern, its values to 1e-15; the references are formed from the
        library's values, which every operator of the case has to repeat bit for bit."""
        assert np.array_equal(rp, self.B.indptr) and np.array_equal(ci, self.B.indices)
        np.testing.assert_allclose(v, self.B.data, rtol=1e-15)
        if self.values is None:
            self.values = v.copy()
            self.values.setflags(write=False)
            self.Bv = sp.csr_matrix((self.values, self.B.indices, self.B.indptr), shape=self.B.shape)
            self.Bl = sp.csr_matrix((self.values.astype(np.longdouble), self.B.indices, self.B.indptr), shape=self.B.shape)
            self.Babs = sp.csr_matrix((np.abs(self.values), self.B.indices, self.B.indptr), shape=self.B.shape)
            self.terms = (np.diff(self.B.indptr) + 2).astype(np.float64)[:, None]
        else:
            assert _same_bits(v, self.values)

    def reference(self, t):
        if t not in self.refs:
            seed = 1000 * sorted(S.CASES).index(self.case) + t
            X = np.random.default_rng(seed).standard_normal((self.N, t))
            Yref = self.Bl @ X.astype(np.longdouble)
            limit = self.terms * U * (self.Babs @ np.abs(X))
            assert Yref.dtype == np.longdouble and np.all(limit > 0)
            scipy_ratio = float(np.max(np.abs(self.Bv @ X - Yref).astype(np.float64) / limit))
            for a in (X, Yref, limit):
                a.setflags(write=False)
            self.refs[t] = (X, Yref, limit, scipy_ratio)
        return self.refs[t]


@functools.lru_cache(maxsize=1)
def _host(case):
    return _Host(case)


def _columns(case):
    return (2, 4, 8, 16) + ((1, 3, 12) if case == "base4" else ())      # (1, 3, 12: column counts off the stride)


@pytest.mark.parametrize("case,switch", S.GPU_SETTINGS, ids=["%s-%s" % cs for cs in S.GPU_SETTINGS])
def test_product_on_multi_slice_blocks(case, switch, monkeypatch):
    import prealps_amd
    _set_switches(monkeypatch, switch)
    h = _host(case)
    prob = prealps_amd.EcgProblem(h.rp, h.ci, h.v, h.P, h.part, scale=True, device=0)
    try:
        assert np.array_equal(prob.rowpos, h.rowpos)
        h.bind(*prob.local_csr())
        failures = []
        for t in _columns(case):
            X, Yref, limit, scipy_ratio = h.reference(t)
            Y = prob.block_operator(X, t)
            got = {k: int(prob.stat(k)) for k in PLAN_STATS}
            want = S.expected(case, t, switch)
            assert got == want, "%s %s t=%d: the plan that ran is %s, the table says %s; %s" % (
                case, switch, t, got, want, _cu_note())
            again = all(_same_bits(Y, prob.block_operator(X, t)) for _ in range(3))
            finite = bool(np.isfinite(Y).all())
            ratio = np.abs(Y - Yref).astype(np.float64) / limit if finite else np.full(Y.shape, np.inf)
            i, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            hist = S.GEOMETRY[(case, S.stride_of(t), switch)][5]
            print("BLOCKS %-6s %-7s t=%-2d | runs %d staged %d slices %d blocks %d (1/2/3/4 slices: %s) stage rows %d = %d B"
                  " | kernel %.3f scipy %.3f of the limit, worst row %d column %d"
                  % (case, switch, t, got["spmm_runs"], got["spmm_staged"], got["spmm_slices"], got["spmm_blocks"],
                     "/".join(str(n) for n in hist), got["spmm_stage_rows"],
                     S.stage_bytes(S.stride_of(t), got["spmm_runs"], got["spmm_stage_rows"]), ratio[i, c], scipy_ratio, i, c))
            sys.stdout.flush()
            assert scipy_ratio <= 1.0                  # (the bound holds for the plainest double-precision product)
            if not finite:
                failures.append("t=%d: the product is not finite" % t)
            elif ratio[i, c] > 1.0:
                failures.append("t=%d: %d entries above the limit, the worst %.3e times (row %d, column %d: %r, reference %r)"
                                % (t, int(np.count_nonzero(ratio > 1.0)), ratio[i, c], i, c, Y[i, c], float(Yref[i, c])))
            if not again:
                failures.append("t=%d: repeated products differ" % t)
        assert not failures, "%s %s: %s" % (case, switch, "; ".join(failures))
    finally:
        prob.close()


# ---- the Gram by-product on four busy wavefronts ------------------------------------------------------------------
GRAM_EXCESS, GRAM_TOL, GRAM_MAX_ITER = 0.02, 1e-5, 60


@functools.lru_cache(maxsize=1)
def _gram_host():
    from oracle import oracle as O
    h = _Host("base4", GRAM_EXCESS)
    ref = O.ECG(h.B, h.rowpos, 4, O.ORTHODIR, O.NO_BS_RED, GRAM_TOL, GRAM_MAX_ITER).solve(O.reference_rhs(h.rowpos))
    return h, int(ref["iters"]), np.array(ref["res"])


def _solve_both_ways(prob, iters, res, tag, monkeypatch):
    """Orthodir t = 4 with the Gram block the SpMM leaves behind and, PREALPS_SPMM_GRAM=0, without it."""
    import prealps_amd
    rhs = prob.reference_rhs()
    for gram in (True, False):
        if not gram:
            monkeypatch.setenv("PREALPS_SPMM_GRAM", "0")
        before = prob.stat("spmm_gram_launches")
        got = prob.solve(rhs, 4, ortho_alg=prealps_amd.ORTHODIR, tol=GRAM_TOL, max_iter=GRAM_MAX_ITER)
        launches = int(prob.stat("spmm_gram_launches") - before)
        n = min(len(got.res), len(res))
        d = np.abs(got.res[:n] - res[:n]) / res[:n]
        print("GRAM %s%s: %d iterations (oracle %d), history within %.2e of the oracle's, %d SpMM launches left the Gram block"
              % (tag, "" if gram else " PREALPS_SPMM_GRAM=0", got.iters, iters, d.max(), launches))
        sys.stdout.flush()
        assert got.iters == iters and len(got.res) == len(res)
        np.testing.assert_allclose(got.res, res, rtol=RTOL_HIST)
        if gram:
            assert launches >= iters, launches
        else:
            assert launches == 0, launches


@pytest.mark.parametrize("switch,env,plan", [
    ("default", {}, (0, 1)),                                   # staged: k_spmm_runs_gram<1>
    ("runs", {"PREALPS_SPMM_RUNS": "2"}, (1, 1)),              # k_spmm_runs_gram<3>
    ("window", {"PREALPS_SPMM_STAGED": "0"}, (0, 0)),          # k_spmm_gram
], ids=["staged", "runs", "window"])
def test_gram_by_product_on_four_busy_wavefronts(switch, env, plan, monkeypatch):
    import prealps_amd
    _set_switches(monkeypatch, "default")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, iters, res = _gram_host()
    assert 15 <= iters < GRAM_MAX_ITER
    prob = prealps_amd.EcgProblem(h.rp, h.ci, h.v, h.P, h.part, scale=True, device=0)
    try:
        prob.create_block_jacobi()
        _solve_both_ways(prob, iters, res, "base4 excess %g %s" % (GRAM_EXCESS, switch), monkeypatch)
        got = {k: int(prob.stat(k)) for k in PLAN_STATS}
        assert got == S.expected("base4", 4, switch), "the plan that ran is %s, the table says %s; %s" % (
            got, S.expected("base4", 4, switch), _cu_note())
        assert (got["spmm_runs"], got["spmm_staged"]) == plan
    finally:
        prob.close()


TINY_TOL = 0.5


@pytest.mark.parametrize("switch", ["default", "runs"])
def test_gram_by_product_of_a_plan_that_stages_less_than_1024_bytes(switch, monkeypatch):
    """60 rows, pentadiagonal, 4 parts: 19 (staged) or 19 + 2 (runs) staged rows of 32 bytes.  With four
    subdomains and t = 4 the iteration terminates exactly at its fourth step: the oracle's residuals are 2.76, 3.45,
    0.390 and then 3e-14, rounding noise that no two implementations share.  tol = 0.5 (||b|| = 1.93) stops after the
    third residual, so the whole history is compared at RTOL_HIST and the Gram block has been used three times."""
    import prealps_amd
    from oracle import oracle as O
    _set_switches(monkeypatch, switch)
    n, P = 60, 4
    A = sp.diags([-1.0, -1.0, 4.0, -1.0, -1.0], [-2, -1, 0, 1, 2], shape=(n, n), format="csr")
    part = O.contiguous_partition(n, P)
    rp, ci, v = O.as_csr(A)
    B, perm, rowpos = O.permute_by_part(O.symrac_scale(A), part, P)
    ref = O.ECG(B, rowpos, 4, O.ORTHODIR, O.NO_BS_RED, TINY_TOL, 1000).solve(O.reference_rhs(rowpos))
    prob = prealps_amd.EcgProblem(rp, ci, v, P, part, scale=True, device=0)
    try:
        before = prob.stat("spmm_gram_launches")
        got = prob.solve(prob.reference_rhs(), 4, ortho_alg=prealps_amd.ORTHODIR, tol=TINY_TOL, max_iter=1000)
        launches = int(prob.stat("spmm_gram_launches") - before)
        stage = int(prob.stat("spmm_stage_rows"))
        print("GRAM pentadiagonal 60 %s: %d iterations (oracle %d), %d staged rows = %d B, %d SpMM launches left the Gram block"
              % (switch, got.iters, ref["iters"], stage, stage * 32, launches))
        assert prob.stat("spmm_staged") == 1.0 and 0 < stage * 32 < 1024
        assert prob.stat("spmm_runs") == (1.0 if switch == "runs" else 0.0)
        assert got.iters == ref["iters"] == 3 and len(got.res) == len(ref["res"])
        np.testing.assert_allclose(got.res, ref["res"], rtol=RTOL_HIST)
        assert launches > 0
    finally:
        prob.close()
