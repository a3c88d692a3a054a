"""The block shapes the SpMM kernels meet on a full device, cut on the host: prealps_amd/csrc/spmm_plan.c alone, built
with gcc into a shared object (no sanitizer: test_spmm_plan_cpu.py runs the builders under ASan + UBSan) and called
through ctypes with cus = 256 for every (case, panel stride, switch setting) of spmm_block_cases.py.

What is asserted: every plan equals the record in spmm_block_cases.GEOMETRY (the numbers test_gpu_spmm_blocks.py
expects of the library's statistics), and the records between them hold every shape the cases exist for -- blocks of
exactly two, three and four slices in staged and run plans, halved beside full blocks, a staging area at its cap, more
than 64 KiB of staging at 8 and 16 columns, a second staging batch, short slices inside a block, window blocks of
several slices.  The last test records why the cases are needed: at 256 compute units the small matrices of
test_gpu_parity.py only ever have one slice per block."""
import numpy as np
import pytest
import scipy.sparse as sp

import spmm_block_cases as S


@pytest.fixture(scope="module")
def plan_library(tmp_path_factory):
    return S.compile_plan_library(tmp_path_factory.mktemp("spmm_blocks"))


@pytest.fixture(scope="module")
def plans(plan_library):
    """Every (case, stride, switch) plan at 256 compute units."""
    out = {}
    for case in S.CASES:
        csr, (_, _, rowpos) = S.matrix(case), S.partition(case)
        for ts in S.STRIDES:
            for switch in S.SWITCHES:
                out[(case, ts, switch)] = S.build_plan(plan_library, csr, rowpos, ts, switch)
    return out


def test_node_graph_matrix_is_what_its_definition_says():
    from prealps_amd import gen
    nn, stride = 500, 37
    for kw in (dict(), dict(far_every=2, nfar=2, excess=0.02), dict(far_every=1, nfar=3)):
        rp, ci, v = gen.node_graph_csr(nn, stride, 1, **kw)
        rp2, ci2, v2 = gen.node_graph_csr(nn, stride, 1, **kw)
        assert np.array_equal(rp, rp2) and np.array_equal(ci, ci2) and np.array_equal(v, v2)
        A = sp.csr_matrix((v, ci, rp), shape=(3 * nn, 3 * nn))
        assert A.has_sorted_indices and (A != A.T).nnz == 0
        G = sp.csr_matrix((np.ones(len(ci)), ci // 3, rp), shape=(3 * nn, nn))[::3]
        G.sum_duplicates()
        assert np.all(G.data == 3) and np.array_equal(np.diff(rp), 3 * np.repeat(np.diff(G.indptr), 3))   # dense 3 x 3 blocks
        G = G.tolil()
        for i in (0, 1, nn // 2, nn - stride - 1):
            assert {i, i + 1, i + stride} <= set(G.rows[i])
        links = (G.tocsr().nnz - nn) // 2           # chain, stride and far links; far ones may coincide or be self links
        nfar = kw.get("nfar", 2) * len(range(0, nn, kw.get("far_every", 7)))
        assert (nn - 1) + (nn - stride) + 0.9 * nfar <= links <= (nn - 1) + (nn - stride) + nfar
        d = A.diagonal()
        off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
        np.testing.assert_allclose(d, (1.0 + kw.get("excess", 1.0)) * off, rtol=1e-14)
        assert np.all(A.data[A.indices != np.repeat(np.arange(3 * nn), np.diff(rp))] < 0)


def _per_block(plan):
    return np.diff(plan["blk_slice"])


def test_every_plan_is_the_recorded_one(plans):
    assert set(plans) == set(S.GEOMETRY)
    for key, plan in sorted(plans.items()):
        assert S.geometry_of(plan) == S.GEOMETRY[key], key
        assert plan["blk_slice"][0] == 0 and plan["blk_slice"][-1] == plan["slices"]
        assert plan["sl_nrows"].sum() == len(S.matrix(key[0])[0]) - 1
    for setting in S.GPU_SETTINGS:
        assert all((setting[0], ts, setting[1]) in S.GEOMETRY for ts in S.STRIDES)


def test_row_counts_are_the_smallest_with_two_three_and_four_slices():
    """block_rows(): a block keeps k slices from 4 * 256 * 64 k rows; every case sits within 384 rows of its edge."""
    for case, want in (("two", 2), ("three", 3), ("base4", 4), ("far2", 4), ("far3", 4), ("ragged", 4)):
        rows = 3 * S.CASES[case][0]
        assert S.nominal_slices(rows) == want and S.nominal_slices(rows - 384) == want - 1, case
        assert 0 <= rows - 4 * S.CUS * 64 * want < 384


@pytest.mark.parametrize("form", ["staged", "runs"])
def test_staged_and_run_plans_have_blocks_of_exactly_two_three_and_four_slices(plans, form):
    for case, k in (("two", 2), ("three", 3), ("base4", 4)):
        for ts in (2, 4) if form == "staged" else S.STRIDES:
            p = plans[(case, ts, form)]
            assert (p["runs"], p["staged"]) == ((1, 1) if form == "runs" else (0, 1))
            per = _per_block(p)
            assert np.count_nonzero(per == k) >= 1024 and np.count_nonzero(per != k) <= 1, (case, ts, per)
    # the plans the library chooses by itself: the run plan at 2 columns, the staged plan at 4
    for case in ("two", "three", "base4"):
        assert plans[(case, 2, "default")]["runs"] == 1 and plans[(case, 4, "default")]["runs"] == 0
        assert plans[(case, 4, "default")]["staged"] == 1


def test_one_launch_mixes_halved_and_full_blocks(plans):
    """A staged block holds fewer slices than block_rows() gives it only at the end of the matrix or after it was
    halved to fit the staging area: far2 has thousands of halved blocks beside full ones, at its cap."""
    for key in (("far2", 4, "default"), ("far2", 4, "staged"), ("far2", 4, "runs"), ("far2", 8, "runs"), ("far2", 16, "runs")):
        p = plans[key]
        per, full = _per_block(p), S.nominal_slices(3 * S.CASES["far2"][0])
        assert full == 4 and p["staged"] == 1
        assert np.count_nonzero(per[:-1] == 2) >= 2000 and np.count_nonzero(per == 4) >= 3, (key, np.bincount(per))
        assert S.stage_cap(key[1], p["runs"]) - 2 <= p["stage_rows"] <= S.stage_cap(key[1], p["runs"])
    # 4 -> 2 -> 1: far3 at 4 columns is halved twice
    for switch in ("staged", "runs"):
        per = _per_block(plans[("far3", 4, switch)])
        assert np.count_nonzero(per[:-1] == 1) >= 4000 and np.count_nonzero(per == 2) >= 4


def test_a_staging_area_is_at_its_cap(plans):
    """Exactly at the cap where a multiple of three rows can be (the staged plan at 8 columns: 768 rows), and one
    node's three rows below it elsewhere."""
    p = plans[("far2", 8, "staged")]
    assert (p["runs"], p["staged"]) == (0, 1) and p["stage_rows"] == S.stage_cap(8, 0) == 768
    for key in (("far2", 4, "staged"), ("far2", 4, "runs"), ("far3", 4, "staged"), ("far3", 4, "runs"),
                ("far2", 8, "runs"), ("far2", 16, "runs")):
        p = plans[key]
        zero_rows = 2 if p["runs"] else 0
        room = S.stage_cap(key[1], p["runs"]) - zero_rows           # 1024 or 1022 rows of X
        assert room in (1022, 1024) and room - 3 < p["stage_rows"] - zero_rows <= room, key
    for key, p in plans.items():
        if p["staged"]:
            assert p["stage_rows"] <= S.stage_cap(key[1], p["runs"]), key


@pytest.mark.parametrize("ts", [8, 16])
def test_run_plans_stage_more_than_64_kib_in_two_batches(plans, ts):
    """launch_spmm sets hipFuncAttributeMaxDynamicSharedMemorySize above 64 KiB; the staging loop takes 512 rows per
    batch at 8 columns (a 16-column panel is worked as two halves of 8)."""
    for case in ("base4", "far2", "ragged"):
        p = plans[(case, ts, "runs")]
        assert p["runs"] == 1 and S.stage_bytes(ts, 1, p["stage_rows"]) == p["stage_rows"] * 80 > 65536, case
        assert p["stage_rows"] > 512
        assert S.stage_bytes(ts, 1, p["stage_rows"]) <= 80 * 1024
    assert plans[("far2", 8, "staged")]["stage_rows"] > 512       # the staged plan at 8 columns: two batches, < 64 KiB
    assert S.stage_bytes(8, 0, plans[("far2", 8, "staged")]["stage_rows"]) <= 65536


def test_short_slices_sit_inside_blocks(plans):
    """Blocks of the staged and run plans span subdomains: with parts cut at random, slices of fewer than 64 rows
    are the first, second and third of four-slice blocks."""
    for key in (("ragged", 2, "runs"), ("ragged", 4, "default"), ("ragged", 4, "runs"), ("ragged", 8, "runs")):
        p = plans[key]
        assert p["staged"] == 1
        first, last = p["blk_slice"][:-1], p["blk_slice"][1:] - 1
        is_last = np.zeros(p["slices"], bool)
        is_last[last] = True
        pos = np.arange(p["slices"]) - np.repeat(first, np.diff(p["blk_slice"]))
        short_inside = (p["sl_nrows"] < 64) & ~is_last
        assert {int(k) for k in pos[short_inside]} == {0, 1, 2}, key
        assert np.count_nonzero(short_inside) >= 1000
        assert p["sl_nrows"].min() < 8


def test_window_plans_have_blocks_of_several_slices(plans):
    for case, hist in (("base4", (0, 683, 0, 683)), ("ragged", (1328, 711, 371, 412)), ("three", (192, 0, 1024, 0))):
        for key in ((case, 8, "default"), (case, 16, "default"), (case, 4, "window")):
            p = plans[key]
            assert (p["runs"], p["staged"]) == (0, 0) and p["win_cap"] == 256
            assert tuple(np.bincount(_per_block(p), minlength=5)[1:5]) == hist
    # a slice that overflows the staging area of a forced staged plan: the window plan takes over
    assert plans[("far3", 16, "staged")]["staged"] == 0 and plans[("far2", 16, "staged")]["staged"] == 0


def _random_spd(n, density, seed):       # (test_gpu_parity.py)
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=rng, format="csr")
    A = M + M.T
    A = sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0))
    A.sort_indices()
    return A


def _contiguous_rowpos(N, P):
    part = np.arange(N, dtype=np.int64) * P // N
    return np.concatenate([[0], np.cumsum(np.bincount(part, minlength=P))]).astype(np.int32)


def test_small_matrices_of_the_parity_tests_only_have_one_slice_blocks(plan_library):
    """Why the cases above exist: on 256 compute units the matrices test_gpu_parity.py checks the product on
    elementwise (elasticity 7^3 in 8 parts, Poisson 12^3 in 5, random 1500 rows in 7) get one slice per block under
    every switch setting and stride, less than 64 KiB of staging and a single staging batch at 8 columns."""
    from prealps_amd import gen
    rp, ci, v = gen.elasticity3d_csr(7)
    prp, pci, pv = gen.poisson3d_csr(12)
    R = _random_spd(1500, 0.004, 11)
    small = (("elasticity7", (rp, ci, v), 8), ("poisson12", (prp, pci, pv), 5),
             ("random1500", (R.indptr.astype(np.int32), R.indices.astype(np.int32), R.data.astype(np.float64)), 7))
    worst = 0
    for name, csr, P in small:
        N = len(csr[0]) - 1
        for ts in S.STRIDES:
            for switch in S.SWITCHES:
                p = S.build_plan(plan_library, csr, _contiguous_rowpos(N, P), ts, switch)
                assert p["blocks"] == p["slices"] and np.all(_per_block(p) == 1), (name, ts, switch)
                worst = max(worst, p["stage_rows"])
    assert worst * 80 < 65536 and worst <= 1024


def test_tiny_matrices_stage_less_than_the_gram_tail_needs(plan_library):
    """spmm_gram_tail hands the four wavefronts' shares over through the first 1024 bytes of the staging area; a
    pentadiagonal matrix of 24 or 60 rows in 4 parts stages less than that at 4 columns, so the launcher has to ask
    for 1024 bytes itself (test_gpu_spmm_blocks.py solves the 60-row system)."""
    for n in (24, 60):
        A = sp.diags([-1.0, -1.0, 4.0, -1.0, -1.0], [-2, -1, 0, 1, 2], shape=(n, n), format="csr")
        csr = (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64))
        for switch in ("default", "runs", "staged"):
            p = S.build_plan(plan_library, csr, _contiguous_rowpos(n, 4), 4, switch)
            assert p["staged"] == 1 and 0 < p["stage_rows"] * 32 < 1024, (n, switch, p["stage_rows"])
