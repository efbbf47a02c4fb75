"""Generate the one-hidden-layer (``--num_layers 1``, main.py's default: the
riverswim recipes) parity fixtures by running the REFERENCE GaussianTrainer and
particle_trainer.ParticleTrainer under make_golden.py's harness (gym stub,
``Adam14`` through ``optimizer_class``, gradient recorder).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_shallow.py

Six fixtures at the recipe shape (obs 1, act 1, hidden [16], B 32), three
steps each, one at (5, 2, [24], 37) with train_bias=False and
use_target_policy, and one reference-written checkpoint.  Runs only where the
read-only reference is present; the .npz / .pt files hold inputs and the
outputs the reference produced on them, nothing else.

Seed condition: a fixture is kept only if the fp32 CPU oracle reproduces the
reference's run under the project's gate (max(1e-5, 3x the reference's own
fp32 distance from the float64 oracle), per key, test_oracle_golden.gated) --
so no hidden unit of the run sits on a ReLU boundary where two correct fp32
sums disagree about the mask, and the GPU tests need no allowance for that.
The parameter seed is advanced until that holds; the seed used is in ``meta``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the oracle package

from make_golden import (Adam14, Box, EPS_LOG, GaussianTrainer, ParticleTrainer, _fill_buffer,  # noqa: E402
                         _producers, _record_batch, gen_det_snapshot, load_sd, pack, save)
import shallow_lib as sl  # noqa: E402
import test_oracle_golden as tog  # noqa: E402


def gen_det(kind, obs_dim, act_dim, hidden, B, steps, n_replay, seed, K=2, delta=0.95, r_min=0.0,
            r_max=5.0, discount=0.99, lr=1e-3, tau=5e-3, idx_seed=1, pi_init_w=0.3, q_init_w=0.3,
            counts=False, mean_update=False, train_bias=True, use_target_policy=False):
    """One run of the reference trainer ``kind`` ('goac' / 'ptrain') as main.py
    builds it (share_layers, deterministic policy; q_min / q_max = r_min /
    r_max / (1 - discount)), for networks of any depth: every gradient, every
    post-step parameter and the statistics of each step."""
    pp, qp = _producers(obs_dim, act_dim, hidden, q_out=K)
    q_min, q_max = r_min / (1 - discount), r_max / (1 - discount)
    torch.manual_seed(0)
    common = dict(action_space=Box(-1, 1, (act_dim,)), discount=discount, reward_scale=1.0,
                  delta=delta, policy_lr=lr, qf_lr=lr, optimizer_class=Adam14,
                  soft_target_tau=tau, target_update_period=1, q_min=q_min, q_max=q_max,
                  share_layers=True, counts=counts, mean_update=mean_update,
                  train_bias=train_bias, use_target_policy=use_target_policy)
    if kind == "goac":
        tr = GaussianTrainer(pp, qp, n_estimators=2, **common)
        assert tr.deterministic
    else:
        tr = ParticleTrainer(pp, qp, n_estimators=K, deterministic=True, **common)
    meta = dict(kind=kind, obs_dim=obs_dim, act_dim=act_dim, hidden=hidden, K=K, B=B, steps=steps,
                n_replay=n_replay, seed=seed, delta=delta, q_min=q_min, q_max=q_max,
                discount=discount, lr=lr, tau=tau, idx_seed=idx_seed, pi_init_w=pi_init_w,
                q_init_w=q_init_w, counts=counts, soft=None, mean_update=mean_update,
                rescale=False, train_bias=train_bias, use_target_policy=use_target_policy)
    if kind == "goac":
        meta.update(standard_bound=float(tr.standard_bound), std_init=float(tr.std_init))
    else:
        meta.update(delta_index=int(tr.delta_index))
    params = sl.params_of(meta)
    qf, tf = tr.qfs[0], tr.tfs[0]
    load_sd(tr.policy, params["policy"])
    load_sd(tr.target_policy, params["target_policy"])
    load_sd(qf, params["qf1"])
    load_sd(tf, params["target_qf1"])
    pol_order, q_order = sl.orders(len(hidden))
    assert list(tr.policy.state_dict()) == pol_order and list(qf.state_dict()) == q_order
    out = {}
    if use_target_policy:   # the DDPG target network: its own weights, recorded
        tpn = sl.params_of(dict(meta, seed=seed + 100))["policy"]
        load_sd(tr.target_policy_network, tpn)
        for pname, t in tr.target_policy_network.state_dict().items():
            out[f"tpn/{pname}"] = t.numpy().copy()
    rb, _ = _fill_buffer(obs_dim, act_dim, n_replay)
    crs = np.random.RandomState(77)
    np.random.seed(idx_seed)
    q_opt = tr.q_optimizer if kind == "goac" else tr.qf_optimizers[0]
    for s in range(steps):
        EPS_LOG.clear()
        batch, idx = _record_batch(rb, B)
        batch = dict(batch)
        if counts:   # about half the rows unvisited, the rest 1..3
            c = crs.randint(0, 4, (B, 1)) * (crs.uniform(0, 1, (B, 1)) < 0.5)
            batch["counts"] = c.astype(np.float64)
            out[f"s{s}/counts"] = batch["counts"][:, 0]
        tr.end_epoch(s)
        tr.train(batch)
        assert len(EPS_LOG) == 0      # deterministic policies draw nothing
        out[f"s{s}/idx"] = idx.astype(np.int64)
        for k, v in tr.get_diagnostics().items():
            out[f"s{s}/stat/{k}"] = np.array(v, np.float64)
        for gname, opt, mod, order in (("policy", tr.policy_optimizer, tr.policy, pol_order),
                                       ("target_policy", tr.target_policy_optimizer,
                                        tr.target_policy, pol_order),
                                       ("qf", q_opt, qf, q_order)):
            assert len(opt.recorded[-1]) == len(order)
            for pname, g in zip(order, opt.recorded[-1]):
                if g is None:   # no gradient: the log-std heads, a frozen bias
                    g = torch.zeros_like(mod.state_dict()[pname])
                pack(out, f"s{s}/grad/{gname}/{pname}", g.numpy(), True)
        for gname, mod in (("policy", tr.policy), ("target_policy", tr.target_policy),
                           ("qf", qf), ("tf", tf)):
            for pname, t in mod.state_dict().items():
                pack(out, f"s{s}/post/{gname}/{pname}", t.numpy(), True)
    return meta, out


def seed_ok(meta, g):
    """The seed condition (module doc); prints the worst keys."""
    errs = sl.oracle_errors(meta, g)
    noise = sl.oracle_errors(meta, g, torch.float64)
    bad = tog.gated(errs, noise)
    w = max(errs.items(), key=lambda kv: kv[1])
    print(f"  seed {meta['seed']}: worst fp32-oracle error {w[1]:.2e} ({w[0]}), "
          f"worst reference noise {max(noise.values()):.2e}, {len(bad)} keys over the gate")
    return not bad


def gen_checked(name, kind, *a, seed0, **kw):
    for seed in range(seed0, seed0 + 20):
        meta, out = gen_det(kind, *a, seed=seed, **kw)
        if seed_ok(meta, {k: np.asarray(v) for k, v in out.items()}):
            save(name, meta, out)
            return
    raise SystemExit(f"{name}: no seed in [{seed0}, {seed0 + 20}) meets the seed condition")


def main():
    torch.set_num_threads(8)
    rs = (1, 1, [16], 32, 3, 400)   # the riverswim recipes' shape
    gen_checked("goac_d1_plain", "goac", *rs, seed0=31)
    gen_checked("goac_d1_counts", "goac", *rs, seed0=33, counts=True)
    gen_checked("goac_d1_mean", "goac", *rs, seed0=35, mean_update=True)
    gen_checked("ptrain_d1_plain", "ptrain", *rs, seed0=37, K=10)
    gen_checked("ptrain_d1_counts", "ptrain", *rs, seed0=39, K=10, counts=True)
    gen_checked("ptrain_d1_mean", "ptrain", *rs, seed0=41, K=10, mean_update=True)
    gen_checked("ptrain_d1_nobias_tpn", "ptrain", 5, 2, [24], 37, 3, 400, seed0=43, K=10,
                train_bias=False, use_target_policy=True)
    gen_det_snapshot(os.path.join(HERE, "goac_d1_snapshot.pt"), "goac", obs_dim=1, act_dim=1,
                     hidden=(16,), B=32)


if __name__ == "__main__":
    main()
