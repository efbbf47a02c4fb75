"""Generate the share_layers=False parity fixtures (the reference trainers'
default: separate one-output critics, each with its own optimizer) by running
the REFERENCE GaussianTrainer and particle_trainer.ParticleTrainer under
make_golden.py's harness (gym stub, ``Adam14`` through ``optimizer_class``, the
gradient recorder of every optimizer).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unshared.py

Ten fixtures of three steps each -- six at the riverswim recipes' shape (obs 1,
act 1, hidden [16], B 32; K = 10 particles), the lqg line's ([8], K = 10), two
at (5, 2, [24], B 37) with train_bias=False, and one whose particles cross --
and one reference-written unshared checkpoint per trainer.  Every critic's
gradients, post-step parameters, target and Adam moments are recorded in full.
Runs only where the read-only reference is present; the .npz / .pt files hold
inputs and the outputs the reference produced on them, nothing else.

Seed conditions (the parameter seed is advanced until both hold; the seed used
and the measured margins are in ``meta``):
 (a) the fp32 CPU oracle (tests/unshared_oracle.py) reproduces the reference's
     run under the project's gate (max(1e-5, 3x the reference's own fp32
     distance from the float64 oracle), per key, test_oracle_golden.gated),
     no element excluded;
 (b) p-oac: in every recorded step the smallest gap between adjacent sorted
     particle values of a row -- critics, target critics, post-step critics --
     is at least 1e-4 of the row's spread, so two correct fp32 sums rank every
     row alike and the GPU tests leave nothing out.
``ptrain_us_crossed`` also needs >= 10 % of step 0's (row, critic) pairs out of
rank: otherwise the rank indicator of the critic gradient is never exercised.
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
                         _plain, _producers, _record_batch, load_sd, pack, save)
import test_oracle_golden as tog  # noqa: E402
import unshared_oracle as uo  # noqa: E402

MIN_GAP = 1e-4


def build(kind, meta, use_automatic_entropy_tuning=False):
    """The reference trainer as main.py builds it without --share_layers
    (one-output producers, main.py:138-143), loaded with the fixture's
    parameters; returns (trainer, critics, targets, critic optimizers)."""
    pp, qp = _producers(meta["obs_dim"], meta["act_dim"], meta["hidden"], q_out=1)
    torch.manual_seed(0)
    common = dict(action_space=Box(-1, 1, (meta["act_dim"],)), discount=meta["discount"],
                  reward_scale=1.0, delta=meta["delta"], policy_lr=meta["lr"], qf_lr=meta["lr"],
                  optimizer_class=Adam14, soft_target_tau=meta["tau"], target_update_period=1,
                  q_min=meta["q_min"], q_max=meta["q_max"], share_layers=False,
                  counts=meta["counts"], mean_update=meta["mean_update"],
                  train_bias=meta["train_bias"], use_target_policy=meta["use_target_policy"],
                  use_automatic_entropy_tuning=use_automatic_entropy_tuning)
    if kind == "goac":
        tr = GaussianTrainer(pp, qp, n_estimators=2, std_lr=meta["std_lr"], **common)
        assert tr.deterministic and tr.qfs == [tr.q, tr.std]
        opts = [tr.q_optimizer, tr.std_optimizer]
    else:
        tr = ParticleTrainer(pp, qp, n_estimators=meta["K"], deterministic=True, **common)
        opts = tr.qf_optimizers
    params = uo.params_of(meta)
    load_sd(tr.policy, params["policy"])
    load_sd(tr.target_policy, params["target_policy"])
    for k in range(uo.n_critics(meta)):
        load_sd(tr.qfs[k], params["qfs"][k])
        load_sd(tr.tfs[k], params["tfs"][k])
        assert list(tr.qfs[k].state_dict()) == uo.Q_ORDER
    assert list(tr.policy.state_dict()) == uo.POL_ORDER
    return tr, opts


def make_meta(kind, obs_dim, act_dim, hidden, B, steps, n_replay, seed, K=2, delta=0.95, r_min=0.0,
              r_max=5.0, discount=0.99, lr=1e-3, std_lr=3e-4, tau=5e-3, idx_seed=1, pi_init_w=0.3,
              q_init_w=0.3, counts=False, mean_update=False, train_bias=True,
              use_target_policy=False):
    q_min, q_max = r_min / (1 - discount), r_max / (1 - discount)
    return dict(kind=kind, obs_dim=obs_dim, act_dim=act_dim, hidden=hidden, K=K, B=B, steps=steps,
                n_replay=n_replay, seed=seed, delta=delta, q_min=q_min, q_max=q_max,
                discount=discount, lr=lr, std_lr=std_lr, tau=tau, idx_seed=idx_seed,
                pi_init_w=pi_init_w, q_init_w=q_init_w, counts=counts, soft=None,
                mean_update=mean_update, rescale=False, train_bias=train_bias,
                use_target_policy=use_target_policy, share_layers=False)


def counts_for(crs, B):
    """About half the rows unvisited, the rest 1..3."""
    return (crs.randint(0, 4, (B, 1)) * (crs.uniform(0, 1, (B, 1)) < 0.5)).astype(np.float64)


def gen(kind, *a, **kw):
    """One run of the reference trainer ``kind`` ('goac' / 'ptrain') with
    share_layers=False: every gradient, post-step parameter, target and Adam
    moment of every network, and the statistics, at each step."""
    meta = make_meta(kind, *a, **kw)
    tr, opts = build(kind, meta)
    if kind == "goac":
        meta.update(standard_bound=float(tr.standard_bound), std_init=float(tr.std_init))
    else:
        meta.update(delta_index=int(tr.delta_index))
    out = {}
    if meta["use_target_policy"]:   # the DDPG target network: its own weights, recorded
        tpn = uo.params_of(dict(meta, seed=meta["seed"] + 100))["policy"]
        load_sd(tr.target_policy_network, tpn)
        for pname, t in tr.target_policy_network.state_dict().items():
            out[f"tpn/{pname}"] = t.numpy().copy()
    rb, _ = _fill_buffer(meta["obs_dim"], meta["act_dim"], meta["n_replay"])
    crs = np.random.RandomState(77)
    np.random.seed(meta["idx_seed"])
    B = meta["B"]
    groups = [("policy", tr.policy_optimizer, tr.policy, uo.POL_ORDER),
              ("target_policy", tr.target_policy_optimizer, tr.target_policy, uo.POL_ORDER)]
    groups += [(f"qf{k}", opts[k], tr.qfs[k], uo.Q_ORDER) for k in range(len(opts))]
    for s in range(meta["steps"]):
        EPS_LOG.clear()
        batch, idx = _record_batch(rb, B)
        batch = dict(batch)
        if meta["counts"]:
            batch["counts"] = counts_for(crs, B)
            out[f"s{s}/counts"] = batch["counts"][:, 0]
        tr.end_epoch(s)
        tr.train(batch)
        assert len(EPS_LOG) == 0      # deterministic policies draw nothing
        out[f"s{s}/idx"] = idx.astype(np.int64)
        for k, v in tr.get_diagnostics().items():
            out[f"s{s}/stat/{k}"] = np.array(v, np.float64)
        for gname, opt, mod, order in groups:
            assert len(opt.recorded[-1]) == len(order) and len(opt.recorded) == s + 1
            params = dict(mod.named_parameters())
            for pname, g in zip(order, opt.recorded[-1]):
                if g is None:   # no gradient: the log-std heads, a frozen bias
                    g = torch.zeros_like(mod.state_dict()[pname])
                pack(out, f"s{s}/grad/{gname}/{pname}", g.numpy(), True)
                pack(out, f"s{s}/post/{gname}/{pname}", mod.state_dict()[pname].numpy(), True)
                if gname.startswith("qf"):
                    st = opt.state.get(params[pname], {})
                    for nm, f in (("m", "exp_avg"), ("v", "exp_avg_sq")):
                        mom = st[f] if st else torch.zeros_like(params[pname])
                        pack(out, f"s{s}/adam_{nm}/{gname}/{pname}", mom.numpy(), True)
        for k, tf in enumerate(tr.tfs):
            for pname, t in tf.state_dict().items():
                pack(out, f"s{s}/post/tf{k}/{pname}", t.numpy(), True)
    return meta, out


def seed_ok(meta, g, crossed):
    """The seed conditions (module doc); prints the worst keys and the margins."""
    extras = {}
    errs = uo.oracle_errors(meta, g, extras=extras)
    noise = uo.oracle_errors(meta, g, torch.float64)
    bad = tog.gated(errs, noise)
    w = max(errs.items(), key=lambda kv: kv[1])
    print(f"  seed {meta['seed']}: worst fp32-oracle error {w[1]:.2e} ({w[0]}), worst reference "
          f"noise {max(noise.values()):.2e}, {len(bad)} keys over the gate, {extras}")
    if bad:
        return False
    if meta["kind"] == "ptrain":
        if extras["min_gap"] < MIN_GAP or (crossed and extras["out_of_rank"] < 0.10):
            return False
        meta.update(min_gap=extras["min_gap"], out_of_rank=extras["out_of_rank"])
    return True


def gen_checked(name, kind, *a, seed0, crossed=False, **kw):
    for seed in range(seed0, seed0 + 40):
        meta, out = gen(kind, *a, seed=seed, **kw)
        if seed_ok(meta, {k: np.asarray(v) for k, v in out.items()}, crossed):
            save(name, meta, out)
            return
    raise SystemExit(f"{name}: no seed in [{seed0}, {seed0 + 40}) meets the seed conditions")


def gen_snapshot(path, kind, K, seed):
    """A checkpoint the reference trainer writes with share_layers=False after
    two counts=True steps, built as main.py builds it (use_automatic_entropy_
    tuning on: the snapshot carries log_alpha and the unused alpha optimizer),
    and the third step it then takes."""
    meta = make_meta(kind, 1, 1, [16], 32, 3, 400, seed, K=K, counts=True)
    tr, _ = build(kind, meta, use_automatic_entropy_tuning=True)
    if kind == "ptrain":
        meta.update(delta_index=int(tr.delta_index))
    rb, _ = _fill_buffer(1, 1, meta["n_replay"])
    crs = np.random.RandomState(5)
    np.random.seed(3)

    def batch_with_counts():
        batch, idx = _record_batch(rb, meta["B"])
        return dict(batch, counts=counts_for(crs, meta["B"])), idx
    for s in range(2):
        batch, _ = batch_with_counts()
        tr.end_epoch(s)
        tr.train(batch)
    snap = _plain(tr.get_snapshot())
    batch, idx = batch_with_counts()
    tr.end_epoch(2)
    tr.train(dict(batch))
    mods = dict(policy=tr.policy, target_policy=tr.target_policy)
    for k in range(uo.n_critics(meta)):
        mods[f"qf{k}"], mods[f"tf{k}"] = tr.qfs[k], tr.tfs[k]
    post = {g: {k: v.detach().clone() for k, v in m.state_dict().items()} for g, m in mods.items()}
    torch.save(dict(meta=meta, snapshot=snap,
                    step3=dict(idx=torch.from_numpy(idx.astype(np.int64)),
                               counts=torch.from_numpy(batch["counts"]), post=post)), path)
    print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1e3:.0f} KB")


def main():
    torch.set_num_threads(8)
    rs = (1, 1, [16], 32, 3, 400)   # the riverswim recipes' shape
    gen_checked("goac_us_plain", "goac", *rs, seed0=51)
    gen_checked("goac_us_counts", "goac", *rs, seed0=53, counts=True)
    gen_checked("goac_us_mean", "goac", *rs, seed0=55, mean_update=True)
    gen_checked("goac_us_nobias", "goac", 5, 2, [24], 37, 3, 400, seed0=57, train_bias=False)
    gen_checked("ptrain_us_plain", "ptrain", *rs, seed0=61, K=10)
    gen_checked("ptrain_us_counts", "ptrain", *rs, seed0=63, K=10, counts=True)
    gen_checked("ptrain_us_mean", "ptrain", *rs, seed0=65, K=10, mean_update=True)
    gen_checked("ptrain_us_lqg", "ptrain", 1, 1, [8], 32, 3, 400, seed0=67, K=10)
    gen_checked("ptrain_us_nobias_tpn", "ptrain", 5, 2, [24], 37, 3, 400, seed0=69, K=3,
                train_bias=False, use_target_policy=True)
    # particles that cross: a prior 1 wide (10 values 0.11 apart) under last-layer
    # weights of +-0.5 on 16 hidden units
    gen_checked("ptrain_us_crossed", "ptrain", *rs, seed0=71, K=10, r_max=0.01, q_init_w=0.5,
                crossed=True)
    gen_snapshot(os.path.join(HERE, "goac_us_snapshot.pt"), "goac", 2, 81)
    gen_snapshot(os.path.join(HERE, "ptrain_us_snapshot.pt"), "ptrain", 10, 83)


if __name__ == "__main__":
    main()
