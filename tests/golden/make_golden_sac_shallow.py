"""Generate the one-hidden-layer SAC / OAC parity fixtures (``--alg oac
--num_layers 1``, main.py's default invocation: oac.sh, sac.sh, the lqg lines
of reproduce.sh) by running the REFERENCE SACTrainer and optimistic_exploration
under make_golden.py's harness (gym stub, ``Adam14`` through ``optimizer_class``,
gradient and eps recorders).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sac_shallow.py

Parameters: fixtures_lib.sac_params(Do, Da, [H], seed, pi_init_w=0.2,
q_init_w=0.1).  Four step fixtures -- every gradient, post-step parameter,
target and Adam moment whole --, two exploration fixtures of 16 observations,
and one reference-written checkpoint.  Runs only where the read-only reference
is present; the .npz / .pt files hold inputs and the outputs the reference
produced on them, nothing else.

Seed condition (step fixtures): a parameter seed is kept only if the fp32 CPU
oracle reproduces the reference's run under parity.gate on every key with no
element left out (sac_shallow_lib.record_errors: plain norm-relative errors, no
Adam sign band, no ReLU-boundary rows) -- so the GPU tests need no allowance
either.  The seed is advanced until that holds; the seed used is in ``meta``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the oracle package

from make_golden import (Adam14, Box, EPS_LOG, SACTrainer, _fill_buffer, _producers,  # noqa: E402
                         _record_batch, _set_adam, _set_alpha, gen_oac_expl, gen_sac_snapshot,
                         load_sd, pack, save)
import sac_shallow_lib as ssl  # noqa: E402
import test_oracle_golden as tog  # noqa: E402
from shallow_lib import orders  # noqa: E402


def gen_sac_d1(obs_dim, act_dim, hidden, B, steps, n_replay, seed, auto_alpha=True, period=1,
               lr=1e-3, tau=5e-3, idx_seed=1, eps_seed=2, mid=None):
    """One run of the reference SACTrainer at one hidden layer.  mid = (t,
    state_seed): the run starts from fixtures_lib.mid_state (Adam moments after
    t steps, log-alpha off its init)."""
    assert len(hidden) == 1
    pol_order, q_order = orders(1)
    pp, qp = _producers(obs_dim, act_dim, hidden)
    torch.manual_seed(0)
    tr = SACTrainer(pp, qp, action_space=Box(-1, 1, (act_dim,)), discount=0.99, reward_scale=1.0,
                    policy_lr=lr, qf_lr=lr, optimizer_class=Adam14, soft_target_tau=tau,
                    target_update_period=period, use_automatic_entropy_tuning=auto_alpha)
    meta = dict(kind="sac", obs_dim=obs_dim, act_dim=act_dim, hidden=hidden, B=B, steps=steps,
                n_replay=n_replay, seed=seed, pi_init_w=0.2, q_init_w=0.1, auto_alpha=auto_alpha,
                log_alpha0=0.0, discount=0.99, reward_scale=1.0, tau=tau, lr=lr, idx_seed=idx_seed,
                eps_seed=eps_seed, target_entropy=-float(act_dim), target_update_period=period)
    if mid is not None:
        meta["mid_state"] = dict(t=mid[0], seed=mid[1])
    params = ssl.params_of(meta)
    for k in ("policy", "qf1", "qf2", "target_qf1", "target_qf2"):
        load_sd(getattr(tr, k), params[k])
    assert list(tr.policy.state_dict()) == pol_order and list(tr.qf1.state_dict()) == q_order
    opts = (("policy", tr.policy_optimizer, pol_order), ("qf1", tr.qf1_optimizer, q_order),
            ("qf2", tr.qf2_optimizer, q_order))
    if auto_alpha:
        tr.log_alpha.data.fill_(0.0)
    ms = ssl.mid_state_of(meta)
    if ms is not None:
        for gname, opt, order in opts:
            _set_adam(opt, order, ms[gname], ms["t"])
        _set_alpha(tr, ms)
        tr._n_train_steps_total = ms["t"]
        meta["log_alpha0"] = float(ms["log_alpha"])
    rb, _ = _fill_buffer(obs_dim, act_dim, n_replay)
    np.random.seed(idx_seed)
    torch.manual_seed(eps_seed)
    out = {}
    for s in range(steps):
        EPS_LOG.clear()
        batch, idx = _record_batch(rb, B)
        tr.end_epoch(s)  # force the eval statistics for this step
        tr.train(dict(batch))
        assert len(EPS_LOG) == 2
        out[f"s{s}/idx"] = idx.astype(np.int64)
        out[f"s{s}/eps1"] = EPS_LOG[0]
        out[f"s{s}/eps2"] = EPS_LOG[1]
        for k, v in tr.get_diagnostics().items():
            out[f"s{s}/stat/{k}"] = np.array(v, np.float64)
        for gname, opt, order in opts:
            assert len(opt.recorded[-1]) == len(order)
            for pname, g, p in zip(order, opt.recorded[-1], opt.param_groups[0]["params"]):
                pack(out, f"s{s}/grad/{gname}/{pname}", g.numpy(), True)
                st = opt.state[p]
                pack(out, f"s{s}/adam/{gname}/{pname}/exp_avg", st["exp_avg"].numpy(), True)
                pack(out, f"s{s}/adam/{gname}/{pname}/exp_avg_sq", st["exp_avg_sq"].numpy(), True)
        if auto_alpha:
            out[f"s{s}/grad/log_alpha"] = tr.alpha_optimizer.recorded[-1][0].numpy()
            out[f"s{s}/post/log_alpha"] = tr.log_alpha.detach().numpy().copy()
        for gname in ("policy", "qf1", "qf2", "target_qf1", "target_qf2"):
            for pname, t in getattr(tr, gname).state_dict().items():
                pack(out, f"s{s}/post/{gname}/{pname}", t.numpy(), True)
    return meta, out


def seed_ok(meta, g):
    """The seed condition (module doc); prints the worst keys."""
    errs = ssl.oracle_errors(meta, g)
    noise = ssl.oracle_noise(meta, g)
    bad = tog.gated(errs, noise)
    w = max(errs.items(), key=lambda kv: kv[1])
    print(f"  seed {meta['seed']}: worst fp32-oracle error {w[1]:.2e} ({w[0]}), "
          f"worst reference noise {max(noise.values()):.2e}, {len(bad)} keys over the gate")
    return not bad


def gen_checked(name, *a, seed0, **kw):
    for seed in range(seed0, seed0 + 20):
        meta, out = gen_sac_d1(*a, seed=seed, **kw)
        if seed_ok(meta, {k: np.asarray(v) for k, v in out.items()}):
            save(name, meta, out)
            return
    raise SystemExit(f"{name}: no seed in [{seed0}, {seed0 + 20}) meets the seed condition")


def main():
    torch.set_num_threads(8)
    gen_checked("sac_d1_riverswim", 1, 1, [16], 32, 3, 400, seed0=51)
    gen_checked("sac_d1_lqg", 1, 1, [8], 32, 3, 400, seed0=53)
    gen_checked("sac_d1_noalpha_period2", 5, 2, [24], 37, 3, 400, seed0=55, auto_alpha=False,
                period=2, tau=0.1)
    gen_checked("sac_d1_mid", 5, 2, [24], 37, 1, 400, seed0=57, mid=(7, 31))
    save("oac_expl_d1_riverswim", *gen_oac_expl("oac_expl_d1_riverswim", 1, 1, [16], 16, 4.66, 23.53,
                                                 seed=61, pi_init_w=0.2, q_init_w=0.1))
    save("oac_expl_d1_small", *gen_oac_expl("oac_expl_d1_small", 5, 2, [24], 16, 4.66, 23.53,
                                             seed=62, pi_init_w=0.2, q_init_w=0.1))
    gen_sac_snapshot(os.path.join(HERE, "sac_d1_snapshot.pt"), obs_dim=1, act_dim=1, hidden=(16,),
                     B=32)


if __name__ == "__main__":
    main()
