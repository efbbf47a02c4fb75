"""The case table of tests/deep_wide_cases.py on the CPU oracles alone (no GPU):
the rows it holds, every row's input conditions at the seed the table stores --
where one fails the row's seed changes, no row and no element is ever left out
-- and the depth-2 kernel branches the table reaches in each step family."""
import numpy as np
import pytest

import deep_wide_cases as dwc

IDS = [r.id for r in dwc.ROWS]


def test_the_table_holds_the_rows_it_should():
    assert dwc.STEP_CASES == dict(
        w30=(4, 3, 30, 17), w50=(11, 9, 50, 33), w36=(5, 16, 36, 48), da32=(17, 32, 64, 19),
        w272=(17, 24, 272, 19), w400=(23, 6, 400, 17), w513=(7, 1, 513, 16),
        humanoid=(376, 17, 256, 37), slabs=(5, 3, 50, 520), b1030n=(5, 6, 36, 1030),
        b1030=(3, 2, 70, 1030))
    assert dwc.FAMILIES == ("sac", "poac", "goac", "ptrain")
    assert len(IDS) == len(set(IDS)) == 4 * 11
    K = dict(w30=2, w50=10, w36=10, da32=3, w272=16, w400=10, w513=10, humanoid=16, slabs=10,
             b1030n=10, b1030=3)
    for n, dims in dwc.STEP_CASES.items():
        for fam in dwc.FAMILIES:
            r = dwc.BY_ID[f"{fam}-{n}"]
            assert (r.Do, r.Da, r.H, r.B) == dims
            assert r.K == dict(sac=None, goac=2).get(fam, K[n]), r.id
            assert dwc.meta_of(r)["hidden"] == [r.H, r.H]
    # 'ptrain': delta_index from delta = 0.95, but for one K = 16 row at delta = 1.0
    last = [r.id for r in dwc.rows_of("ptrain") if r.delta != dwc.DELTA]
    assert last == ["ptrain-w272"]
    for r in dwc.rows_of("ptrain"):
        want = r.K - 1 if r.id in last else dwc.delta_index(r.K, 0.95)
        assert dwc.meta_of(r)["delta_index"] == want, r.id
    assert dwc.meta_of(dwc.BY_ID["ptrain-w272"])["delta_index"] == 15
    assert dwc.meta_of(dwc.BY_ID["ptrain-humanoid"])["delta_index"] == 14
    assert (dwc.MARGIN, dwc.T_MID, dwc.TANH_MAX) == (8.0, 7, 0.999)
    assert sorted(dwc.SEEDS) == sorted(IDS)
    for r in dwc.ROWS:   # a bounded search: 20 seeds, 100 for the slab and large-batch rows
        assert r.max_seeds == (100 if r.name in ("slabs", "b1030n", "b1030") else 20)
        assert r.base_seed <= r.seed < r.base_seed + r.max_seeds, r.id
        assert r.H >= 4 and 1 <= r.Da <= 32 and r.B <= 1030


@pytest.mark.parametrize("row_id", IDS)
def test_input_conditions_hold_at_the_stored_seed(row_id):
    """1. no hidden unit of either layer of any evaluation the step makes has
    |pre_float64| below 8 x that layer's largest |pre_fp32 - pre_float64| (no
    ReLU mask can differ between correct fp32 evaluations, so no element is
    left out of any comparison); 2. particle rows: the smallest rank gap of the
    critic outputs exceeds the same 8 x discrepancy (the sorted ranks cannot
    differ); 3. every policy action stays below 0.999 in float64."""
    r = dwc.BY_ID[row_id]
    c = dwc.stored_conditions(row_id)
    print(f"{row_id}: seed {r.seed}, smallest |pre| / b {c['mask']:.2f}, rank gap / b {c['rank']:.3g}, "
          f"largest |a| {c['tanh']:.4f}")
    assert np.isfinite(c["mask"]) and c["mask"] > 1.0, c
    assert c["rank"] > 1.0, c
    assert r.particles == np.isfinite(c["rank"])
    assert c["tanh"] < dwc.TANH_MAX, c


def _have(family, **want):
    """Some row of the family reaches every one of the given values together."""
    for r in dwc.rows_of(family):
        got = dwc.reaches(r)
        if all(got[k] == v for k, v in want.items()):
            return r.id
    return None


@pytest.mark.parametrize("family", dwc.FAMILIES)
def test_branch_coverage_of_the_step_table(family):
    """Every depth-2 branch the issue names occurs in a row of every family that
    has it (dwc.reaches restates the constants of head.hip, rows.hip and the plans)."""
    hit = {}

    def need(name, **want):
        hit[name] = _have(family, **want)
        assert hit[name], (family, name, want)

    # head.hip's launch forms (:254-258 NT, :281-287 KS)
    for nt in (1, 2, 3, 4):
        need(f"NT = {nt}", NT=nt)
    need("NT = 2 with KS = 5", NT=2, KS=5)
    need("KS = 8 at NT = 3", NT=3, KS=8)
    need("KS = 8 at NT = 4", NT=4, KS=8)
    need("Da = 16: every lane of the tile live", Da=16, NT=2)
    need("Da = 1", Da=1, NT=1, KS=2)
    need("5 column chunks", col_chunks=5, cols_per_chunk=55)
    need("7 column chunks", col_chunks=7, cols_per_chunk=58)
    need("9 column chunks of 57", col_chunks=9, cols_per_chunk=57)
    # the head product's k loop (head.hip:84-117, :157): its tail group at H % 4 != 0
    need("tail overlap below one tile", head_tail_overlap=True, head_k_chunks=2)
    need("tail overlap over four k-chunks", head_tail_overlap=True, head_k_chunks=4)
    need("17 k-chunks: a second pass", head_k_chunks=17, head_tail_overlap=False)
    need("33 k-chunks with an odd width", head_k_chunks=33, odd_width=True)
    # row_heads / row_heads2 (rows.hip:316, :337-366)
    need("the one-batch form (the control)", heads_path="fast", heads_chunks=16)
    need("generic loop, scalar tail below one tile", heads_path="generic", heads_tail="scalar",
         heads_chunks=2)
    need("generic loop, float4 tail", heads_path="generic", heads_tail="float4", heads_chunks=3)
    need("generic loop, second pass", heads_path="generic", heads_passes=2, heads_tail="none")
    need("generic loop, third pass with a scalar tail", heads_path="generic", heads_passes=3,
         heads_tail="scalar")
    # the GEMM tiles with H % 4 != 0 (an odd leading dimension of the hidden activations)
    need("gemm_small, odd ld", gemm="small", odd_ld=True, fused=True)
    need("slabs and the unfused Adam, odd ld", gemm="small", odd_ld=True, fused=False)
    need("gemm.hip at large batch, H % 8 = 4", gemm="lds_tiled", mult4_only=True, ragged_rows=True)
    need("gemm_fwd / gemm_bwdp at large batch, odd ld, two ragged column tiles", gemm="fwd_bwdp",
         odd_ld=True, ragged_col_tiles=2, ragged_rows=True)
    need("a ragged third row block", row_blocks=3, ragged_rows=True)
    need("whole row blocks", row_blocks=3, ragged_rows=False)
    need("exactly one row block", row_blocks=1, ragged_rows=False)
    if family == "sac":    # head_dh2 (sac_plan.hip:480-487) by the shape alone
        need("head_dh2 on at its last Da", head_dh2=True, Da=24)
        need("head_dh2 off by Da", head_dh2=False, head_dh2_off_by="Da")
        need("head_dh2 off by width", head_dh2=False, head_dh2_off_by="H")
    if family == "poac":   # the H & 3 fallbacks (particle_plan.hip:68-70, 222-233; plan_api.hip:362)
        need("rank-K dX stay GEMM launches", dx_gemm_launches=True, large_batch=False)
        need("the same at large batch, sp_ql not tied to sp_q0", dx_gemm_launches=True,
             sp_ql_tied=False, large_batch=True)
        need("sp_ql tied (the control)", sp_ql_tied=True)
        need("particle_min_kernel's generic loop, scalar tail", min_kernel_path="generic",
             heads_tail="scalar")
        need("particle_min_kernel's generic loop, third pass", min_kernel_path="generic", heads_passes=3)
    if family in ("poac", "ptrain"):   # the sort / rank kernels
        need("K = 16: every sort16 slot live", sort_K=16)
        need("K = 3", sort_K=3)
        need("K = 2", sort_K=2)
        need("K = 10", sort_K=10)
    if family == "ptrain":
        need("the last sorted slot", sort_K=16, delta_index=15)
    # head.hip:280 kp4 needs 17 (net, tile) pairs: two nets over more than 128 columns of one
    # chunk, i.e. SAC at B >= 1024 and H > 128 -- no row of the issue's table (its large-batch
    # rows are 36 and 70 wide: wider ones meet no seed, see the table's comment)
    assert not any(dwc.reaches(r)["kp4"] for r in dwc.rows_of(family))
    for k, v in hit.items():
        print(f"{family}: {k}: {v}")
