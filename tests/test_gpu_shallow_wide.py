"""The one-hidden-layer gradient steps over the widths and action counts of
tests/shallow_wide_cases.py: ShallowSACTrainer (csrc/sac_shallow_plan.hip), the
shared depth-1 g-oac / p-oac step and the separate-critic step
(csrc/det_plan.hip) through the branches of csrc/rows.hip and csrc/head.hip
that the narrow fixtures never run -- a second kDshChunk, Dp = 4 and 16, the
second accumulator for Da > 16, row_heads' 16-chunk and generic forms, several
head column chunks, partial seg_last_update workgroups.

Per row: one step from a mid-training state (non-zero Adam moments, t = 7); every
gradient, post-step parameter, Adam moment and Polyak target (SAC: log-alpha and
its gradient too) whole against the fp32 CPU oracle run from the trainer's own
pre-step state.  No element is left out: the rows' inputs keep every ReLU
pre-activation and particle rank clear of fp32 rounding
(tests/test_shallow_wide_cases_cpu.py).  The gate is parity.gate: 1e-5, or 3x the
fp32 oracle's distance from the float64 oracle on the same inputs and state."""
import numpy as np
import pytest
import torch

import parity
import sac_shallow_lib as ssl
import shallow_lib as sl
import shallow_wide_cases as swc
import unshared_oracle as uo

pytestmark = pytest.mark.gpu


def _plan_facts(tr):
    from oac_amd import _lib
    L, h = _lib.lib(), tr._last_plan.handle
    return bool(L.oac_sac_trace(h, 0) & _lib.TRACE["fused"]), L.oac_sac_launch_count(h)


def _gated(got, r32, r64, what):
    """{key: (error, gate)} of the GPU's tensors over their gates; prints the
    worst error over its gate."""
    assert sorted(got) == sorted(r32) == sorted(r64)
    errs = {k: parity.rel_err(got[k], r32[k]) for k in r32}
    gates = {k: parity.gate(k, parity.rel_err(r32[k], r64[k])) for k in r32}
    w = max(errs, key=lambda k: errs[k] / gates[k])
    print(f"{what}: worst {w} {errs[w]:.2e} (gate {gates[w]:.2e}), {errs[w] / gates[w]:.3f} of it; "
          f"widest gate {max(gates.values()):.2e}; {len(errs)} tensors")
    return {k: (errs[k], gates[k]) for k in errs if not errs[k] <= gates[k]}


@pytest.mark.parametrize("row_id", [r.id for r in swc.rows_of("sac")])
def test_sac_shallow_step(row_id):
    row = swc.BY_ID[row_id]
    meta = swc.meta_of(row)
    tr = swc.trainer_of(row)
    assert tr.n_hidden == 1 and tr._n_train_steps_total == swc.T_MID
    batch, e1, e2 = swc.batch_of(row)
    bad = ssl.step_against_oracle(tr, meta, batch, e1, e2, row_id)
    fused, n = _plan_facts(tr)
    want = swc.reaches(row)["fused"]
    assert fused == want and n == (7 if want else 9), (fused, n)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:10]


def _det_step(row):
    meta = swc.meta_of(row)
    tr = swc.trainer_of(row)
    assert tr.n_hidden == 1 and tr.unshared == row.unshared and tr._n_train_steps_total == swc.T_MID
    if row.kind == "ptrain":
        assert tr.delta_index == meta["delta_index"]
    b, _, _ = swc.batch_of(row)
    lib = uo if row.unshared else sl
    o32 = lib.oracle_from_gpu(tr, meta, dtype=torch.float32)
    o64 = lib.oracle_from_gpu(tr, meta, dtype=torch.float64)
    tr.train_from_torch(b)
    torch.cuda.synchronize()
    out32, out64 = o32.step(b), o64.step(b)
    if row.unshared:
        got = uo.step_tensors(o32, None, meta, tr=tr)
        r32, r64 = uo.step_tensors(o32, out32, meta), uo.step_tensors(o64, out64, meta)
    else:
        got = sl.step_tensors(o32, None, tr=tr)
        r32, r64 = sl.step_tensors(o32, out32), sl.step_tensors(o64, out64)
    assert all(np.isfinite(v).all() for v in got.values())
    return tr, _gated(got, r32, r64, row.id)


@pytest.mark.parametrize("row_id", [r.id for r in swc.rows_of("shared")])
def test_shared_depth_1_step(row_id):
    row = swc.BY_ID[row_id]
    tr, bad = _det_step(row)
    fused, n = _plan_facts(tr)
    reach = swc.reaches(row)
    if reach["fused"]:     # (the slab and large-batch rows: as test_gpu_shallow.py, the values alone)
        assert fused and n == 8, (fused, n)
    else:
        assert not fused
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:10]


@pytest.mark.parametrize("row_id", [r.id for r in swc.rows_of("separate")])
def test_separate_critics_step(row_id):
    row = swc.BY_ID[row_id]
    tr, bad = _det_step(row)
    assert len(tr.qfs) == row.K
    fused, n = _plan_facts(tr)
    if swc.reaches(row)["fused"]:
        assert fused and n == 9, (fused, n)
    else:                  # (as test_gpu_unshared.py's slab rows: the slab reduction, the unfused Adam)
        assert not fused and n > 9, (fused, n)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:10]
