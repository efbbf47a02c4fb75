"""Generate the DDPG parity fixtures by running the REFERENCE DDPGTrainer
(/root/reference/trainer/ddpg_trainer.py) under make_golden.py's harness: the
gym stub, ``Adam14`` through the trainer's ``optimizer_class`` argument (torch
1.4 semantics, so ``policy_loss.backward()`` after the critic's step sees the
post-step critic) and the gradient recorder.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ddpg.py

Runs only where the read-only reference is present; the .npz / .pt files hold
inputs and the outputs the reference produced on them, nothing else.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the oracle package

from make_golden import (Adam14, Box, EPS_LOG, FlattenMlp, TanhGaussianPolicy, _fill_buffer,  # noqa: E402
                         _plain, _record_batch, load_sd, pack, save)
from trainer.ddpg_trainer import DDPGTrainer  # noqa: E402
from ddpg_oracle import LOG_STD_KEYS, POLICY_KEYS, ddpg_params  # noqa: E402
from fixtures_lib import PARAM_ORDER_Q  # noqa: E402


def _producers(obs_dim, act_dim, hidden, std):
    """main.py:143-149: --alg ddpg builds TanhGaussianPolicy(std = std * ones)."""
    def policy_producer(**kw):
        return TanhGaussianPolicy(hidden_sizes=hidden, obs_dim=obs_dim, action_dim=act_dim,
                                  std=None if std is None else np.ones(act_dim) * std)

    def q_producer(**kw):
        return FlattenMlp(input_size=obs_dim + act_dim, output_size=1, hidden_sizes=hidden)
    return policy_producer, q_producer


def _trainer(meta):
    pp, qp = _producers(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["std"])
    torch.manual_seed(0)
    tr = DDPGTrainer(pp, qp, action_space=Box(-1, 1, (meta["act_dim"],)),
                     discount=meta["discount"], reward_scale=meta["reward_scale"],
                     policy_lr=meta["lr"], qf_lr=meta["lr"], optimizer_class=Adam14,
                     soft_target_tau=meta["tau"], target_update_period=meta["period"],
                     use_target_policy=meta["use_target_policy"])
    params = ddpg_params(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["seed"],
                         pi_init_w=meta["pi_init_w"], q_init_w=meta["q_init_w"],
                         log_std_head=meta["std"] is None)
    load_sd(tr.policy, params["policy"])
    load_sd(tr.qf, params["qf"])
    load_sd(tr.target_qf, params["target_qf"])
    if meta["use_target_policy"]:   # the constructor's tau-1 copy was of the producer's init
        load_sd(tr.target_policy_network, params["policy"])
    return tr, params


def gen_ddpg(name, obs_dim, act_dim, hidden, B, steps, n_replay, full, seed=21, std=None,
             pi_init_w=1e-3, q_init_w=3e-3, discount=0.99, reward_scale=1.0, tau=1e-2, lr=1e-3,
             idx_seed=1, period=1, use_target_policy=False, own_tpn=False):
    meta = dict(kind="ddpg", obs_dim=obs_dim, act_dim=act_dim, hidden=hidden, B=B, steps=steps,
                n_replay=n_replay, seed=seed, std=std, pi_init_w=pi_init_w, q_init_w=q_init_w,
                discount=discount, reward_scale=reward_scale, tau=tau, lr=lr, idx_seed=idx_seed,
                period=period, use_target_policy=use_target_policy)
    tr, params = _trainer(meta)
    pol_order = POLICY_KEYS + (LOG_STD_KEYS if std is None else [])
    assert list(tr.policy.state_dict()) == pol_order
    out = {}
    if own_tpn:   # its own weights, recorded: a frozen network is then not the policy
        load_sd(tr.target_policy_network, params["tpn"])
        for pname, t in tr.target_policy_network.state_dict().items():
            out[f"tpn/{pname}"] = t.numpy().copy()
    rb, _ = _fill_buffer(obs_dim, act_dim, n_replay)
    np.random.seed(idx_seed)
    for s in range(steps):
        EPS_LOG.clear()
        batch, idx = _record_batch(rb, B)
        tr.end_epoch(s)
        tr.train(dict(batch))
        assert len(EPS_LOG) == 0      # the deterministic policy draws nothing
        out[f"s{s}/idx"] = idx.astype(np.int64)
        for k, v in tr.get_diagnostics().items():
            out[f"s{s}/stat/{k}"] = np.array(v, np.float64)
        for gname, opt, order, mod in (("policy", tr.policy_optimizer, pol_order, tr.policy),
                                       ("qf", tr.qf_optimizer, PARAM_ORDER_Q, tr.qf)):
            for pname, g in zip(order, opt.recorded[-1]):
                if g is None:
                    g = torch.zeros_like(mod.state_dict()[pname])
                pack(out, f"s{s}/grad/{gname}/{pname}", g.numpy(), full)
        for gname, mod in (("policy", tr.policy), ("qf", tr.qf), ("tf", tr.target_qf)):
            for pname, t in mod.state_dict().items():
                pack(out, f"s{s}/post/{gname}/{pname}", t.numpy(), full)
        if use_target_policy:
            # the reference's soft update of it onto itself (t (1 - tau) + t tau in
            # fp32) moves nothing but the last bit of some elements
            ref = params["tpn"] if own_tpn else params["policy"]
            for pname, t in tr.target_policy_network.state_dict().items():
                assert np.allclose(t.numpy(), ref[pname], rtol=1e-6, atol=0), pname
    return meta, out


def gen_ddpg_snapshot(path, obs_dim=11, act_dim=3, hidden=(32, 32), B=16, seed=23):
    """The reference DDPGTrainer's checkpoint (ddpg_trainer.py:203-217; std =
    0.1, use_target_policy) after two steps, as plain tensors with
    target_policy_network as its state dict, and the third step it then
    takes."""
    meta = dict(kind="ddpg", obs_dim=obs_dim, act_dim=act_dim, hidden=list(hidden), B=B, steps=3,
                n_replay=300, seed=seed, std=0.1, pi_init_w=0.2, q_init_w=0.1, discount=0.99,
                reward_scale=1.0, tau=1e-2, lr=1e-3, idx_seed=3, period=1, use_target_policy=True)
    tr, _ = _trainer(meta)
    rb, _ = _fill_buffer(obs_dim, act_dim, 300)
    np.random.seed(3)
    pre_idx = []
    for s in range(2):
        batch, idx = _record_batch(rb, B)
        pre_idx.append(torch.from_numpy(idx.astype(np.int64)))
        tr.end_epoch(s)
        tr.train(dict(batch))
    snap = tr.get_snapshot()
    snap["target_policy_network"] = snap["target_policy_network"].state_dict()
    snap = _plain(snap)
    batch, idx = _record_batch(rb, B)
    tr.end_epoch(2)
    tr.train(dict(batch))
    mods = dict(policy=tr.policy, qf=tr.qf, tf=tr.target_qf)
    post = {g: {k: v.detach().clone() for k, v in m.state_dict().items()} for g, m in mods.items()}
    fixture = dict(meta=meta, snapshot=snap, pre_idx=pre_idx,
                   step3=dict(idx=torch.from_numpy(idx.astype(np.int64)), post=post))
    torch.save(fixture, path)
    print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1e3:.0f} KB")


def main():
    save("ddpg_small", *gen_ddpg("ddpg_small", 111, 8, [32, 32], 32, 3, 500, True,
                                 pi_init_w=0.3, q_init_w=0.3))
    save("ddpg_fixed_std", *gen_ddpg("ddpg_fixed_std", 11, 3, [16, 16], 16, 3, 200, True, std=0.1,
                                     pi_init_w=0.5, q_init_w=0.5))
    save("ddpg_tpn", *gen_ddpg("ddpg_tpn", 11, 3, [16, 16], 16, 3, 200, True, std=0.1,
                               pi_init_w=0.5, q_init_w=0.5, period=2, use_target_policy=True,
                               own_tpn=True))
    save("ddpg_stress", *gen_ddpg("ddpg_stress", 11, 3, [32, 32], 16, 3, 300, True,
                                  pi_init_w=0.7, q_init_w=0.3, reward_scale=2.0, discount=0.95,
                                  tau=0.01, lr=1e-3))
    save("ddpg_humanoid", *gen_ddpg("ddpg_humanoid", 376, 17, [256, 256], 256, 2, 20000, False,
                                    std=0.1, use_target_policy=True))
    gen_ddpg_snapshot(os.path.join(HERE, "ddpg_snapshot.pt"))


if __name__ == "__main__":
    main()
