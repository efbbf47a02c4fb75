"""The case table of tests/shallow_wide_cases.py on the CPU oracles alone (no
GPU): every row's input conditions at the seed the table stores -- where one
fails the row's seed changes, no row and no element is ever left out -- and the
kernel branches the table reaches in each step family."""
import numpy as np
import pytest

import shallow_wide_cases as swc

IDS = [r.id for r in swc.ROWS]


def test_the_table_holds_the_rows_it_should():
    assert swc.STEP_CASES == dict(
        w64=(3, 3, 64, 17), w68=(4, 4, 68, 16), da9=(11, 9, 128, 33), da16=(5, 16, 32, 48),
        w252=(23, 6, 252, 37), da32=(17, 32, 260, 19), humanoid=(376, 17, 256, 37),
        w512=(376, 17, 512, 19), slabs=(23, 6, 68, 600))
    assert swc.PTRAIN_K == dict(w64=10, w68=10, da9=10, da16=10, w252=10, humanoid=16, da32=3,
                                w512=5, slabs=5)
    for n in swc.STEP_CASES:
        for fam in ("sac", "goac", "ptrain"):
            assert f"{fam}-{n}" in swc.BY_ID
        assert swc.BY_ID[f"goac-{n}"].K == 2 and swc.BY_ID[f"ptrain-{n}"].K == swc.PTRAIN_K[n]
    sep = {(r.family, (r.Do, r.Da, r.H, r.B), r.K) for r in swc.rows_of("separate")}
    assert {("us_goac", (376, 17, 256, 37), 2), ("us_ptrain", (23, 6, 60, 37), 10),
            ("us_ptrain", (5, 16, 20, 33), 16), ("us_ptrain", (17, 32, 88, 19), 3)} <= sep
    # the large-batch kernel set once per family that has it (SAC_SHALLOW refuses B >= 1024)
    for grp, n in (("sac", 0), ("shared", 2), ("separate", 1)):
        assert sum(swc.reaches(r)["large_batch"] for r in swc.rows_of(grp)) == n
    assert sorted(swc.SEEDS) == sorted(IDS)
    for r in swc.ROWS:   # a bounded search, like gen_checked's
        assert r.base_seed <= r.seed < r.base_seed + swc.MAX_SEEDS, r.id
        assert r.H % 4 == 0 and 1 <= r.Da <= 32


@pytest.mark.parametrize("row_id", IDS)
def test_input_conditions_hold_at_the_stored_seed(row_id):
    """1. no hidden unit of any evaluation the step makes has |pre_float64|
    below 8 x that evaluation's largest |pre_fp32 - pre_float64| (no ReLU mask
    can differ between correct fp32 evaluations, so no element is left out of
    any comparison); 2. particle rows: the smallest rank gap of the critic
    outputs exceeds the same 8 x discrepancy (the sorted ranks cannot differ);
    3. every policy action stays below 0.999 in float64."""
    r = swc.BY_ID[row_id]
    c = swc.stored_conditions(row_id)
    print(f"{row_id}: seed {r.seed}, smallest |pre| / b {c['mask']:.2f}, rank gap / b {c['rank']:.3g}, "
          f"largest |a| {c['tanh']:.4f}")
    assert np.isfinite(c["mask"]) and c["mask"] > 1.0, c
    assert c["rank"] > 1.0, c
    assert (r.kind == "ptrain") == np.isfinite(c["rank"])
    assert c["tanh"] < swc.TANH_MAX, c


def _have(group, **want):
    """Some row of the group reaches every one of the given values together."""
    for r in swc.rows_of(group):
        got = swc.reaches(r)
        if all(got[k] == v for k, v in want.items()):
            return r.id
    return None


@pytest.mark.parametrize("group", ["sac", "shared"])
def test_branch_coverage_of_the_step_table(group):
    """Every branch value the issue names occurs in a row of the family
    (swc.reaches restates the constants of rows.hip and the plans)."""
    hit = {}

    def need(name, **want):
        hit[name] = _have(group, **want)
        assert hit[name], (group, name, want)

    # the lane split of the two backward kernels (rows.hip:1019-1023, 1306-1310)
    need("Dp = 4", Dp=4)
    need("Dp = 16, clamped lanes", Dp=16, lanes_live=9, acc1_lanes=0)
    need("Dp = 16, every lane live, acc1 idle", Dp=16, lanes_live=16, acc1_lanes=0)
    need("acc1 for one lane", acc1_lanes=1)
    need("acc1 for all 16 lanes", acc1_lanes=16)
    # the kDshChunk = 256 loop (rows.hip:975, 1025, 1318)
    need("exactly one full chunk", n_chunks=1, last_chunk=256)
    need("a second chunk of 4 units (< 16 lanes)", n_chunks=2, last_chunk=4)
    need("two full chunks", n_chunks=2, last_chunk=256)
    # row_heads (rows.hip:316, 337)
    need("fast path, 8 chunks", heads_path="fast", heads_chunks=8)
    need("fast path, all 16 chunks", heads_path="fast", heads_chunks=16)
    need("generic path past 256", heads_path="generic", heads_chunks=17)
    need("H % 16 != 0 past 64", heads_path="generic", heads_chunks=5)
    # launch_policy_head's column chunks (sac_shallow_plan.hip:128, det_plan.hip:486)
    need("last width with one column chunk", col_chunks=1, cols_per_chunk=64)
    need("two column chunks of 34", col_chunks=2, cols_per_chunk=34)
    need("63-column chunks", col_chunks=4, cols_per_chunk=63)
    need("the widest layer: 8 column chunks", col_chunks=8, cols_per_chunk=64)
    # the GEMM roles: tiles of 32 (gemm_small.hip), widths that are multiples of 4 only
    need("H a multiple of 4 only, partial last GEMM tile", mult4_only=True, partial_gemm_tile=True,
         heads_chunks=16)
    need("ragged second row block", row_blocks=2, ragged_rows=True)
    # split-K slabs and the unfused Adam at a ragged width past 64 (plan_common.h:66-78)
    need("slabs", fused=False, large_batch=False, cols_per_chunk=34)
    if group == "shared":
        need("large-batch kernel set", large_batch=True, col_chunks=2, ragged_rows=True)
    for k, v in hit.items():
        print(f"{group}: {k}: {v}")


def test_branch_coverage_of_the_separate_critic_table():
    hit = {}

    def need(name, **want):
        hit[name] = _have("separate", **want)
        assert hit[name], (name, want)

    # the stacked width K H is what the row kernels and the head launch see
    assert sorted(r.width for r in swc.rows_of("separate")) == [136, 264, 320, 512, 600]
    need("stacked 512 at Humanoid dims: two full chunks", n_chunks=2, last_chunk=256, acc1_lanes=1)
    need("stacked 600: a third chunk of 88", n_chunks=3, last_chunk=88)
    # rows.hip:1082 nbw = ceil(K H / 64), the last workgroup's columns
    need("seg_last_update: 10 column workgroups, the last with 24", seg_workgroups=10, seg_last_cols=24)
    need("stacked 320 with Dp = 16", n_chunks=2, last_chunk=64, Dp=16, lanes_live=16)
    need("stacked 264: acc1 live, a second chunk of 8", n_chunks=2, last_chunk=8, acc1_lanes=16)
    need("wide-critic head form past 320", col_chunks=10)
    need("large-batch kernel set", large_batch=True, col_chunks=2)
    r600 = swc.BY_ID["us_ptrain-s600"]   # the 256 and 512 boundaries fall inside segments 4 and 8
    assert 256 // r600.H == 4 and 256 % r600.H and 512 // r600.H == 8 and 512 % r600.H
    assert max(r.Da for r in swc.rows_of("separate")) > 5
    for k, v in hit.items():
        print(f"separate: {k}: {v}")
