"""The small-batch GEMM kernel's roles and launch header (csrc/gemm_small.hip).

A launch's workgroups take their role -- tile, fused-optimizer side block,
row-copy / eps side block -- and their task from the launch header alone, and
a tile block requests the StepState words of adam_consts with its task record,
long before the epilogue that uses them.  None of that may change a result:

* the index-slot form of the drop-in step (256 < B <= 1024: the step's indices
  in the host slot that batch_counter names, not in the kernel arguments)
  against the device-ring path on the same indices, bit for bit;
* ragged tiles with every role in one step (partial row and column tiles,
  fused-Adam epilogues, shadow copy blocks, the fold and head-dX instances)
  against the fp32 oracle at 1e-5, direct launches against the captured graph
  bit for bit;
* the Adam constants off the published path (t > 1 from a snapshot, Polyak
  period 2, the data-parallel phase calls whose first launch does not publish
  the step's bias corrections) against the oracle / the single-call step;
* alpha (log_alpha, its Adam m / v, its gradient) after each of those steps
  (test_gpu_teacher._sac_compare gates them with every other tensor).

Reference: trainer/trainer.py:126-224, rl_algorithm.py:160-167.
"""
import ctypes

import numpy as np
import pytest
import torch

import parity
from gpu_helpers import batch_from, sac_trainer_for
from oracle import sac_oracle as so
from test_gpu_teacher import (_dropin_step, _np_sd, _replay_for, _sac_compare,
                              sac_oracle_from_gpu)

pytestmark = pytest.mark.gpu


def _meta(B, hidden, **kw):
    m = dict(obs_dim=7, act_dim=5, hidden=[hidden, hidden], seed=3, pi_init_w=0.2, q_init_w=0.1,
             discount=0.99, reward_scale=1.0, lr=3e-4, tau=5e-3, auto_alpha=True, log_alpha0=0.0,
             n_replay=2000, B=B)
    m.update(kw)
    return m


def _state(tr):
    torch.cuda.synchronize()
    return torch.cat([tr.params, tr.targets, tr.alpha_state[:3]]).cpu().numpy()


def _eps(meta, s):
    rs = np.random.RandomState(100 + s)
    shape = (meta["B"], meta["act_dim"])
    return rs.standard_normal(shape).astype(np.float32), rs.standard_normal(shape).astype(np.float32)


def _idx(meta, s):
    return np.random.RandomState(200 + s).randint(0, meta["n_replay"], meta["B"])


def _teacher_step(tr, meta, s, name):
    """One teacher-forced step (test_gpu_teacher's protocol): the oracle takes
    the GPU trainer's own pre-step state, both take the step, every tensor --
    gradients, parameters, Adam m / v, targets, log_alpha and its Adam state --
    is gated at 1e-5."""
    orc = sac_oracle_from_gpu(tr, meta)
    pre = {grp: _np_sd(getattr(tr, grp)) for grp in ("qf1", "qf2", "policy")}
    batch = batch_from(meta, _idx(meta, s))
    e1, e2 = _eps(meta, s)
    tr.end_epoch(s)
    tr.train_from_torch(batch, eps1=e1, eps2=e2)
    torch.cuda.synchronize()
    out = orc.step(so.NumpyReplay.to_torch(batch), e1, e2)
    _sac_compare(tr, orc, out, pre, batch, meta, name, s)


def test_index_slot_dropin_equals_device_ring():
    """B = 288: the drop-in step reads its rows through the host index slot
    (rows = ring + (batch_counter % slots) * B; batch_counter requested with
    the task record).  3 train() steps from rb.random_batch against
    train_from_ring on the same indices: bitwise.  (_dropin_step checks the
    in-step gather against rb._storage[idx] bit for bit.)"""
    meta = _meta(288, 32)
    B = meta["B"]
    a = sac_trainer_for(meta)
    rb = _replay_for(meta)
    np.random.seed(5)
    idx = [_dropin_step(a, rb, meta)[0] for _ in range(3)]
    b = sac_trainer_for(meta)
    ring = torch.from_numpy(np.concatenate(idx).astype(np.int32)).to(rb._storage.device)
    b.train_from_ring(rb._storage, ring, 3, B, n_steps=3)
    sa, sb = _state(a), _state(b)
    assert np.isfinite(sa).all()
    assert np.array_equal(sa, sb)


def test_ragged_tiles_every_role_against_oracle():
    """B = 37, hidden 40: tiles_n = 2 with a partial column tile, a partial
    row tile, fused-Adam epilogues, shadow copy blocks, the fold and head-dX
    launches.  3 teacher-forced steps at 1e-5 per tensor."""
    meta = _meta(37, 40)
    tr = sac_trainer_for(meta)
    for s in range(3):
        _teacher_step(tr, meta, s, "small_roles/ragged")


def test_ragged_tiles_direct_equals_graph():
    meta = _meta(37, 40)
    out = []
    for graph in (False, True):
        tr = sac_trainer_for(meta, use_graph=graph)
        for s in range(3):
            e1, e2 = _eps(meta, s)
            tr.train_from_torch(batch_from(meta, _idx(meta, s)), eps1=e1, eps2=e2)
        torch.cuda.synchronize()
        out.append(torch.cat([tr.params, tr.targets, tr.adam_m, tr.adam_v,
                              tr.alpha_state[:3]]).cpu().numpy())
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[0], out[1])


def _restored(meta, t):
    """A trainer restored from a snapshot taken at step count t (non-zero Adam
    moments from one real step, then the count set to t)."""
    src = sac_trainer_for(meta)
    e1, e2 = _eps(meta, 9)
    src.train_from_torch(batch_from(meta, _idx(meta, 9)), eps1=e1, eps2=e2)
    torch.cuda.synchronize()
    ss = src.get_snapshot()
    ss["_n_train_steps_total"] = t
    for k in ("policy_optim_state_dict", "qf1_optim_state_dict", "qf2_optim_state_dict",
              "alpha_optim_state_dict"):
        for st in ss[k]["state"].values():
            st["step"] = t
    tr = sac_trainer_for(meta)
    tr.restore_from_snapshot(ss)
    assert tr._n_train_steps_total == t
    return tr


def test_adam_constants_from_snapshot_across_polyak_periods():
    """target_update_period = 2, restored at t = 7: 4 steps (t = 8..11) cover
    a Polyak step and a non-Polyak step twice; m, v, targets and alpha at 1e-5
    against the oracle on every step."""
    meta = _meta(37, 40, target_update_period=2)
    tr = _restored(meta, 7)
    for s in range(4):
        _teacher_step(tr, meta, s, "small_roles/period2_t7")
    assert tr._n_train_steps_total == 11


def test_phase_calls_take_the_pow_branch():
    """oac_sac_step_phase (the data-parallel phases at world size 1): the first
    launch of a phase is not the step's publishing launch, so the optimizers
    see bc_t != t and evaluate the bias corrections with pow.  One step by
    phases against the single-call step from the same state: 1e-5 per tensor."""
    from oac_amd import _lib
    meta = _meta(37, 40, target_update_period=2)
    batch = batch_from(meta, _idx(meta, 0))
    e1, e2 = _eps(meta, 0)
    outs = []
    for phases in (False, True):
        tr = _restored(meta, 7)
        tr.train_from_torch(batch, eps1=e1, eps2=e2)   # t = 8: the plan, this batch in its workspace
        torch.cuda.synchronize()
        if phases:
            plan = tr._last_plan
            sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for ph in (0, 1, 2, 3):
                _lib.check(_lib.lib().oac_sac_step_phase(plan.handle, ph, _lib.OAC_STEP_DEVICE_EPS, sp))
        else:
            tr.train_from_torch(batch)                 # t = 9, device Philox eps
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in
                     dict(params=tr.params, targets=tr.targets, m=tr.adam_m, v=tr.adam_v,
                          alpha=tr.alpha_state[:3]).items()})
    errs = {k: parity.rel_err(outs[1][k], outs[0][k]) for k in outs[0]}
    print("phase calls vs single call:", errs)
    assert all(np.isfinite(v).all() for v in outs[1].values())
    assert not {k: e for k, e in errs.items() if e > 1e-5}, errs
