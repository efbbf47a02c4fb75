"""The two-hidden-layer gradient steps over the widths, action counts and head
counts of tests/deep_wide_cases.py: SACTrainer (csrc/sac_plan.hip),
ParticleTrainerOAC (csrc/particle_plan.hip) and the shared-critic
GaussianTrainer / ParticleTrainer (csrc/det_plan.hip) through the branches of
csrc/head.hip, csrc/rows.hip and the GEMM kernels that the fixtures' widths
(multiples of 4 up to 256) never run -- the head product's tail at H % 4 != 0,
NT = 2 and 4, KS = 8, Da = 1, five to nine column chunks, row_heads' generic
loop with its float4 and scalar tails and its second and third pass, the
H & 3 fallbacks of the P-OAC plan, head_dh2 switched off by the shape, hidden
activations with an odd leading dimension on every GEMM kernel, K = 2, 3, 16.

Per row: one step from a mid-training state (non-zero Adam moments, t = 7); every
gradient, post-step parameter, Adam moment and Polyak target (SAC / P-OAC:
log-alpha, its gradient and its moments too) whole against the fp32 CPU oracle
run from the trainer's own pre-step state.  No element is left out: the rows'
inputs keep every ReLU pre-activation of both layers and every particle rank
clear of fp32 rounding (tests/test_deep_wide_cases_cpu.py).  The gate is
parity.gate: 1e-5, or 3x the fp32 oracle's distance from the float64 oracle on
the same inputs and state; nothing in it comes from the GPU's result."""
import numpy as np
import pytest
import torch

import deep_wide_cases as dwc
import sac_shallow_lib as ssl
import shallow_lib as sl
from oracle import sac_oracle as so
from test_gpu_shallow_wide import _gated, _plan_facts
from test_gpu_teacher import poac_oracle_from_gpu, sac_oracle_from_gpu

pytestmark = pytest.mark.gpu


def _alpha_tensors(rec, orc=None, out=None, tr=None):
    """log-alpha, its gradient and its Adam moments: the oracle's, or the
    trainer's (alpha_state: value, m, v, ..., gradient at 5)."""
    if tr is not None:
        a = tr.alpha_state.detach().cpu().double().numpy()
        vals = (a[5:6], a[0:1], a[1:2], a[2:3])
    else:
        vals = (out["grads"]["log_alpha"], orc.log_alpha, orc.opt_a.m["log_alpha"],
                orc.opt_a.v["log_alpha"])
        vals = tuple(v.detach().double().numpy().reshape(1) for v in vals)
    for k, v in zip(("grad/log_alpha", "post/log_alpha", "adam/log_alpha/exp_avg",
                     "adam/log_alpha/exp_avg_sq"), vals):
        rec[k] = np.array(v, np.float64)
    return rec


def _sac_tensors(meta, orc=None, out=None, tr=None):
    rec = ssl.gpu_tensors(meta, tr) if tr is not None else ssl.oracle_tensors(meta, orc, out)
    return _alpha_tensors(rec, orc, out, tr)


def _poac_tensors(orc=None, out=None, tr=None):
    """sac_shallow_lib's keys for the P-OAC step's groups: policy, the shared
    critic and its Polyak target."""
    from gpu_helpers import module_tensors
    cpu = lambda t: t.detach().cpu().double().numpy().copy()
    rec = {}
    groups = (("policy", getattr(orc, "P", None), getattr(orc, "opt_p", None), tr.policy if tr else None),
              ("qf", getattr(orc, "Q", None), getattr(orc, "opt_q", None), tr.qfs[0] if tr else None))
    for grp, params, opt, mod in groups:
        if tr is not None:
            srcs = (module_tensors(tr, mod, tr.grads), mod.state_dict(),
                    module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v))
            names = [n for n, _ in mod.named_parameters()]
        else:
            srcs, names = (out["grads"][grp], params, opt.m, opt.v), list(params)
        for pn in names:
            for what, src in zip(("grad", "post", "adam_m", "adam_v"), srcs):
                rec[f"{what}/{grp}/{pn}"] = cpu(src[pn])
    for pn, t in (tr.tfs[0].state_dict() if tr is not None else orc.T).items():
        rec[f"post/tf/{pn}"] = cpu(t)
    return _alpha_tensors(rec, orc, out, tr)


def _step(row):
    """(trainer, {key: (error, gate)} of the tensors over their gate) after one
    step of the trainer and of both oracles from the trainer's pre-step state."""
    meta = dwc.meta_of(row)
    tr = dwc.trainer_of(row)
    assert tr._n_train_steps_total == dwc.T_MID
    b, e1, e2 = dwc.batch_of(row)
    if row.det:
        if row.family == "ptrain":
            assert tr.delta_index == meta["delta_index"]
        o32 = sl.oracle_from_gpu(tr, meta, dtype=torch.float32)
        o64 = sl.oracle_from_gpu(tr, meta, dtype=torch.float64)
        tr.train_from_torch(b)
        torch.cuda.synchronize()
        out32, out64 = o32.step(b), o64.step(b)
        got = sl.step_tensors(o32, None, tr=tr)
        r32, r64 = sl.step_tensors(o32, out32), sl.step_tensors(o64, out64)
    else:
        from_gpu = sac_oracle_from_gpu if row.family == "sac" else poac_oracle_from_gpu
        o32, o64 = from_gpu(tr, meta, torch.float32), from_gpu(tr, meta, torch.float64)
        assert float(o32.log_alpha) != 0.0 and float(o32.opt_a.v["log_alpha"]) > 0.0
        tr.train_from_torch(b, eps1=e1, eps2=e2)
        torch.cuda.synchronize()
        out32, out64 = o32.step(b, e1, e2), o64.step(b, e1, e2)
        if row.family == "sac":
            got = _sac_tensors(meta, tr=tr)
            r32, r64 = _sac_tensors(meta, o32, out32), _sac_tensors(meta, o64, out64)
        else:
            got = _poac_tensors(tr=tr)
            r32, r64 = _poac_tensors(o32, out32), _poac_tensors(o64, out64)
    assert so.n_hidden(o32.P) == 2
    assert all(np.isfinite(v).all() for v in got.values()), [k for k, v in got.items()
                                                            if not np.isfinite(v).all()]
    return tr, _gated(got, r32, r64, row.id)


def _worst(bad):
    return sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:10]


@pytest.mark.parametrize("row_id", [r.id for r in dwc.rows_of("sac")])
def test_sac_step(row_id):
    from oac_amd import _lib
    row = dwc.BY_ID[row_id]
    tr, bad = _step(row)
    reach = dwc.reaches(row)
    bits = _lib.lib().oac_sac_trace(tr._last_plan.handle, 0)
    assert bool(bits & _lib.TRACE["fused"]) == reach["fused"], bits
    assert bool(bits & _lib.TRACE["head_dh2"]) == reach["head_dh2"], bits
    assert not bad, _worst(bad)


@pytest.mark.parametrize("row_id", [r.id for r in dwc.rows_of("poac")])
def test_particle_oac_step(row_id):
    row = dwc.BY_ID[row_id]
    tr, bad = _step(row)   # (the P-OAC plan sets no trace bit for its Adam form: the values alone)
    assert tr.num_particles == row.K
    assert not bad, _worst(bad)


@pytest.mark.parametrize("row_id", [r.id for r in dwc.rows_of("goac") + dwc.rows_of("ptrain")])
def test_shared_critic_step(row_id):
    row = dwc.BY_ID[row_id]
    tr, bad = _step(row)
    fused, _ = _plan_facts(tr)
    assert fused == dwc.reaches(row)["fused"], fused
    assert not bad, _worst(bad)
