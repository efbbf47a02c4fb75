"""Generate the policy-ensemble parity fixtures by running the REFERENCE
particle_trainer.ParticleTrainer with ``ensemble=True`` and its own
``EnsemblePolicy`` (share_layers=False, deterministic policies, one hidden
layer) under make_golden.py's harness (gym stub, ``Adam14`` through
``optimizer_class``, the gradient recorder of every optimizer).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ensemble.py

Four fixtures of three steps each -- three at the w_oac recipe's shape (obs 2,
act 1, hidden [16], B 32, K = 10 particles, P = 5 policies: plain, counts,
mean_update) and ``ens_ragged`` (5, 3, [24], B 37, K 3, P 3, train_bias=False),
whose act_dim > 1 exercises the constructor's initial-action draw -- and one
reference-written checkpoint.  Every policy's and critic's gradient, post-step
parameters and Adam moments are recorded whole, with the policy chosen for each
next_obs row, the target critics' values on the chosen actions and the
statistics.  ``ens_ragged`` also records 64 observations with the reference's
``get_action(deterministic=True)``, the per-policy proposals, their upper
bounds and ``forward``'s six outputs, on its final state.  Runs only where the
read-only reference is present; the .npz / .pt files hold inputs and the
outputs the reference produced on them, nothing else.

Seed conditions (the parameter seed is advanced until all hold; the seed and
the measured margins are in ``meta``):
 (a) the fp32 CPU oracle (tests/ensemble_oracle.py) reproduces the recording
     under the project's gate (test_oracle_golden.gated), no element excluded;
 (b) wherever K values are sorted -- critics, target critics, every proposal of
     the selection and of the policy step -- adjacent sorted values of a row are
     at least 1e-4 of the row's spread apart;
 (c) in every row where a selection happens the best and the second-best UB_p
     are at least 1e-4 of the row's spread of UB_p apart (the recorded
     observations included);
 (d) ``ens_plain``, step 0: at least two policies are each chosen on >= 10 % of
     the rows -- otherwise the argmax is never exercised.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the oracle package

from make_golden import (Adam14, Box, EPS_LOG, FlattenMlp, ParticleTrainer, _fill_buffer, _plain,  # noqa: E402
                         _record_batch, load_sd, pack, save)
from make_golden_unshared import counts_for  # noqa: E402
from trainer.policies import EnsemblePolicy, TanhGaussianPolicy  # noqa: E402
import test_oracle_golden as tog  # noqa: E402
import ensemble_oracle as eo  # noqa: E402

N_OBS = 64


def _producers(meta, calls):
    """main.py:44-106 at one output per critic; ``calls`` receives the keyword
    arguments of every policy_producer call."""
    Do, Da, hidden = meta["obs_dim"], meta["act_dim"], meta["hidden"]

    def policy_producer(deterministic=False, bias=None, ensemble=False, n_policies=1,
                        approximator=None, share_layers=False):
        calls.append(dict(bias=bias, ensemble=ensemble, n_policies=n_policies,
                          share_layers=share_layers))
        if ensemble:
            return EnsemblePolicy(approximator=approximator, hidden_sizes=hidden, obs_dim=Do,
                                  action_dim=Da, n_policies=n_policies, bias=bias,
                                  share_layers=share_layers)
        return TanhGaussianPolicy(hidden_sizes=hidden, obs_dim=Do, action_dim=Da, bias=bias)

    def q_producer(bias=None, positive=False, train_bias=True):
        return FlattenMlp(input_size=Do + Da, output_size=1, hidden_sizes=hidden, bias=bias,
                          positive=positive, train_bias=train_bias)
    return policy_producer, q_producer


def build(meta, use_automatic_entropy_tuning=False):
    calls = []
    pp, qp = _producers(meta, calls)
    torch.manual_seed(0)
    np.random.seed(meta["np_seed"])   # (act_dim > 1: the constructor draws the initial actions)
    tr = ParticleTrainer(pp, qp, n_estimators=meta["K"], deterministic=True,
                         action_space=Box(-1, 1, (meta["act_dim"],)), discount=meta["discount"],
                         reward_scale=1.0, delta=meta["delta"], policy_lr=meta["lr"],
                         qf_lr=meta["lr"], optimizer_class=Adam14, soft_target_tau=meta["tau"],
                         target_update_period=1, q_min=meta["q_min"], q_max=meta["q_max"],
                         share_layers=False, ensemble=True, n_policies=meta["P"],
                         counts=meta["counts"], mean_update=meta["mean_update"],
                         train_bias=meta["train_bias"],
                         use_automatic_entropy_tuning=use_automatic_entropy_tuning)
    ens_call = [c for c in calls if c["ensemble"]]
    assert len(ens_call) == 1 and [c["ensemble"] for c in calls] == [False, True, False]
    meta["initial_actions"] = [float(v) for v in ens_call[0]["bias"]]
    meta["delta_index"] = int(tr.delta_index)
    # the quirk: policy i's mean-head bias is arctanh(initial_actions[i]) in every dimension
    for i, pol in enumerate(tr.policy.policies):
        want = np.full(meta["act_dim"], np.arctanh(meta["initial_actions"][i]), np.float32)
        assert np.array_equal(pol.last_fc.bias.detach().numpy(), want)
    params = eo.params_of(meta)
    for i, pol in enumerate(tr.policy.policies):
        load_sd(pol, params["policies"][i])
        assert list(pol.state_dict()) == eo.POL_ORDER
    load_sd(tr.target_policy, params["target_policy"])
    for k in range(meta["K"]):
        load_sd(tr.qfs[k], params["qfs"][k])
        load_sd(tr.tfs[k], params["tfs"][k])
    return tr


def make_meta(obs_dim, act_dim, hidden, B, steps, n_replay, seed, K, P, delta=0.95, r_min=0.0,
              r_max=5.0, discount=0.99, lr=1e-3, tau=5e-3, idx_seed=1, pi_init_w=0.3, q_init_w=0.3,
              counts=False, mean_update=False, train_bias=True):
    q_min, q_max = r_min / (1 - discount), r_max / (1 - discount)
    return dict(kind="ptrain", obs_dim=obs_dim, act_dim=act_dim, hidden=hidden, K=K, P=P, B=B,
                steps=steps, n_replay=n_replay, seed=seed, np_seed=seed + 1000, delta=delta,
                q_min=q_min, q_max=q_max, discount=discount, lr=lr, tau=tau, idx_seed=idx_seed,
                pi_init_w=pi_init_w, q_init_w=q_init_w, counts=counts, soft=None,
                mean_update=mean_update, rescale=False, train_bias=train_bias,
                use_target_policy=False, share_layers=False, ensemble=True)


def watch_selection(tr, log):
    """Record which policy EnsemblePolicy.forward chose per row: the returned
    action is gathered from the per-policy results, so it equals exactly one
    proposal (checked)."""
    orig = tr.policy.forward

    def forward(obs, reparameterize=True, deterministic=False, return_log_prob=False):
        res = orig(obs, reparameterize, deterministic, return_log_prob)
        with torch.no_grad():
            props = torch.stack([p(obs, deterministic=True)[0] for p in tr.policy.policies], dim=0)
            hit = (props == res[0][None]).all(dim=2)                     # [P, B]
            assert bool(hit.any(dim=0).all())
            log.append((hit.int().argmax(dim=0).numpy().astype(np.int64), res[0].detach().clone()))
        return res
    tr.policy.forward = forward


def record_state(out, s, tr, groups):
    for gname, opt, mod, order in groups:
        assert len(opt.recorded[-1]) == len(order) and len(opt.recorded) == s + 1
        params = dict(mod.named_parameters())
        for pname, g in zip(order, opt.recorded[-1]):
            if g is None:   # no gradient: the log-std heads, a frozen bias
                g = torch.zeros_like(mod.state_dict()[pname])
            pack(out, f"s{s}/grad/{gname}/{pname}", g.numpy(), True)
            pack(out, f"s{s}/post/{gname}/{pname}", mod.state_dict()[pname].numpy(), True)
            st = opt.state.get(params[pname], {})
            for nm, f in (("m", "exp_avg"), ("v", "exp_avg_sq")):
                mom = st[f] if st else torch.zeros_like(params[pname])
                pack(out, f"s{s}/adam_{nm}/{gname}/{pname}", mom.numpy(), True)
    for k, tf in enumerate(tr.tfs):
        for pname, t in tf.state_dict().items():
            pack(out, f"s{s}/post/tf{k}/{pname}", t.numpy(), True)


def gen(*a, acting=False, **kw):
    meta = make_meta(*a, **kw)
    tr = build(meta)
    assert len(tr.policy_optimizers) == meta["P"] and len(tr.policy_optimizer.recorded) == 0
    out = {}
    rb, _ = _fill_buffer(meta["obs_dim"], meta["act_dim"], meta["n_replay"])
    crs = np.random.RandomState(77)
    np.random.seed(meta["idx_seed"])
    B = meta["B"]
    groups = [(f"policy{p}", tr.policy_optimizers[p], tr.policy.policies[p], eo.POL_ORDER)
              for p in range(meta["P"])]
    groups.append(("target_policy", tr.target_policy_optimizer, tr.target_policy, eo.POL_ORDER))
    groups += [(f"qf{k}", tr.qf_optimizers[k], tr.qfs[k], eo.Q_ORDER) for k in range(meta["K"])]
    chosen = []
    watch_selection(tr, chosen)
    for s in range(meta["steps"]):
        EPS_LOG.clear()
        del chosen[:]
        batch, idx = _record_batch(rb, B)
        batch = dict(batch)
        if meta["counts"]:
            batch["counts"] = counts_for(crs, B)
            out[f"s{s}/counts"] = batch["counts"][:, 0]
        # the next actions the step is about to use, on the pre-step networks
        nobs = torch.from_numpy(batch["next_observations"]).float()
        tr.end_epoch(s)
        with torch.no_grad():
            if meta["mean_update"]:
                a2 = tr.target_policy(nobs, deterministic=True)[0]
            else:
                a2 = tr.policy(obs=nobs, deterministic=True)[0]
                pre_sel = chosen[-1][0].copy()
                del chosen[:]
            tq = torch.stack([t(nobs, a2)[:, 0] for t in tr.tfs], dim=0)       # [K, B]
        out[f"s{s}/tq"] = tq.numpy().copy()
        tr.train(batch)
        assert len(EPS_LOG) == 0      # deterministic policies draw nothing
        if meta["mean_update"]:
            assert not chosen
        else:
            assert len(chosen) == 1 and np.array_equal(chosen[0][0], pre_sel)
            assert torch.equal(chosen[0][1], a2)
            out[f"s{s}/sel"] = chosen[0][0]
        out[f"s{s}/idx"] = idx.astype(np.int64)
        for k, v in tr.get_diagnostics().items():
            out[f"s{s}/stat/{k}"] = np.array(v, np.float64)
        record_state(out, s, tr, groups)
    assert len(tr.policy_optimizer.recorded) == 0   # SACTrainer's optimizer is never stepped
    if acting:
        obs = np.random.RandomState(meta["seed"] + 7).standard_normal((N_OBS, meta["obs_dim"]))
        out["act/obs"] = obs
        with torch.no_grad():
            acts = np.stack([tr.policy.get_action(o, deterministic=True)[0] for o in obs])
            props = np.stack([tr.policy.get_actions(obs, deterministic=True, index=i)
                              for i in range(meta["P"])])
            ubs = np.stack([tr.predict(obs, props[i]).numpy()[:, 0] for i in range(meta["P"])])
            del chosen[:]
            six = tr.policy(obs=torch.from_numpy(obs).float(), deterministic=True)
        out["act/get_action"] = acts
        out["act/proposals"], out["act/ub"] = props, ubs
        out["act/sel"] = chosen[0][0]
        for nm, t in zip(("action", "mean", "log_std", "log_prob", "std", "pre_tanh"), six):
            out[f"act/forward/{nm}"] = t.numpy().copy()
        # (one row at a time against all 64 at once: equal up to fp32 rounding)
        assert np.allclose(acts, out["act/forward/action"], rtol=0, atol=1e-6)
    return meta, out


def seed_ok(name, meta, g):
    extras = {}
    try:
        errs = eo.oracle_errors(meta, g, extras=extras)
    except AssertionError as e:   # (a chosen index differs: a selection margin too small)
        print(f"  seed {meta['seed']}: {e}")
        return False
    noise = eo.oracle_errors(meta, g, torch.float64)
    bad = tog.gated(errs, noise)
    w = max(errs.items(), key=lambda kv: kv[1])
    print(f"  seed {meta['seed']}: worst fp32-oracle error {w[1]:.2e} ({w[0]}), worst reference "
          f"noise {max(noise.values()):.2e}, {len(bad)} keys over the gate, {extras}")
    if bad or extras["min_gap"] < eo.MIN_GAP:
        return False
    if not meta["mean_update"] and extras["sel_gap"] < eo.MIN_GAP:
        return False
    if name == "ens_plain" and sum(v >= 0.10 for v in extras["chosen_share"]) < 2:
        return False
    if "act/obs" in g:
        params = {"policies": [{pn: g[f"s{meta['steps'] - 1}/post/policy{p}/{pn}"]
                                for pn in eo.POL_ORDER} for p in range(meta["P"])],
                  "qfs": [{pn: g[f"s{meta['steps'] - 1}/post/qf{k}/{pn}"] for pn in eo.Q_ORDER}
                          for k in range(meta["K"])]}
        base = eo.params_of(meta)
        params.update(policy=params["policies"][0], target_policy=base["target_policy"],
                      tfs=base["tfs"])
        act = eo.make_oracle(meta, params=params).act(g["act/obs"])
        if not np.array_equal(act["sel"].numpy(), g["act/sel"]) or act["sel_gap"] < eo.MIN_GAP:
            return False
        extras["act_sel_gap"] = act["sel_gap"]
    meta.update({k: v for k, v in extras.items()})
    return True


def gen_checked(name, *a, seed0, **kw):
    for seed in range(seed0, seed0 + 40):
        meta, out = gen(*a, seed=seed, **kw)
        if seed_ok(name, meta, {k: np.asarray(v) for k, v in out.items()}):
            save(name, meta, out)
            return
    raise SystemExit(f"{name}: no seed in [{seed0}, {seed0 + 40}) meets the seed conditions")


def gen_snapshot(path, seed0):
    """A checkpoint the reference trainer writes with ensemble=True after two
    steps, built as main.py builds it (use_automatic_entropy_tuning on), and
    the third step it then takes -- at the first seed whose three steps keep
    the margins (b) and (c) on the oracle's run of the same batches."""
    for seed in range(seed0, seed0 + 40):
        meta = make_meta(2, 1, [16], 32, 3, 400, seed, K=10, P=5)
        tr = build(meta, use_automatic_entropy_tuning=True)
        orc = eo.make_oracle(meta)
        rb, _ = _fill_buffer(2, 1, meta["n_replay"])
        np.random.seed(3)
        gaps = []
        for s in range(3):
            if s == 2:
                snap = _plain(tr.get_snapshot())
                moments = [[dict(m=opt.state[p]["exp_avg"].clone(), v=opt.state[p]["exp_avg_sq"].clone())
                            if p in opt.state else None for p in opt.param_groups[0]["params"]]
                           for opt in tr.policy_optimizers]
            batch, idx = _record_batch(rb, meta["B"])
            out = orc.step(dict(batch))
            gaps.append(min(out["min_gap"], out["sel_gap"]))
            tr.end_epoch(s)
            tr.train(dict(batch))
        print(f"  seed {seed}: margins {gaps}")
        if min(gaps) >= eo.MIN_GAP:
            break
    else:
        raise SystemExit("ens_snapshot: no seed meets the margins")
    meta["margins"] = gaps
    assert isinstance(snap["policy_state_dict"], list) and len(snap["policy_state_dict"]) == 5
    assert "policy_optims_state_dicts" not in snap and not snap["policy_optim_state_dict"]["state"]
    mods = {f"policy{p}": m for p, m in enumerate(tr.policy.policies)}
    mods["target_policy"] = tr.target_policy
    for k in range(meta["K"]):
        mods[f"qf{k}"], mods[f"tf{k}"] = tr.qfs[k], tr.tfs[k]
    post = {g: {k: v.detach().clone() for k, v in m.state_dict().items()} for g, m in mods.items()}
    torch.save(dict(meta=meta, snapshot=snap, policy_moments=moments,
                    step3=dict(idx=torch.from_numpy(idx.astype(np.int64)), post=post)), path)
    print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1e3:.0f} KB")


def main():
    torch.set_num_threads(8)
    if sys.argv[1:] == ["snapshot"]:
        return gen_snapshot(os.path.join(HERE, "ens_snapshot.pt"), 99)
    rs = (2, 1, [16], 32, 3, 400)   # the w_oac recipe's shape
    gen_checked("ens_plain", *rs, seed0=91, K=10, P=5)
    gen_checked("ens_counts", *rs, seed0=93, K=10, P=5, counts=True)
    gen_checked("ens_mean", *rs, seed0=95, K=10, P=5, mean_update=True)
    gen_checked("ens_ragged", 5, 3, [24], 37, 3, 400, seed0=97, K=3, P=3, train_bias=False,
                acting=True)
    gen_snapshot(os.path.join(HERE, "ens_snapshot.pt"), 99)


if __name__ == "__main__":
    main()
