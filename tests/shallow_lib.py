"""Shared pieces of the one-hidden-layer (``--num_layers 1``) tests of the
g-oac GaussianTrainer and the p-oac ParticleTrainer: parameter orders for a
given depth, the CPU oracle for a fixture, its errors against a golden (as
test_oracle_golden.det_errors, which is written for two layers), and the
oac_amd trainer for a fixture.  Used by tests/golden/make_golden_shallow.py
(the seed condition), the CPU oracle test and the GPU tests."""
import numpy as np
import torch

import parity
import test_oracle_golden as tog
from fixtures_lib import goac_params, ptrain_params
from gpu_helpers import Space, StateDictModule
from oracle import sac_oracle as so

FIXTURES = ["goac_d1_plain", "goac_d1_counts", "goac_d1_mean",
            "ptrain_d1_plain", "ptrain_d1_counts", "ptrain_d1_mean",
            "ptrain_d1_nobias_tpn"]


def orders(n_hidden):
    """(policy, critic) state_dict key orders of the reference at this depth
    (networks.py:42-53, trainer/policies.py:241-243)."""
    fcs = [f"fc{i}.{w}" for i in range(n_hidden) for w in ("weight", "bias")]
    last = ["last_fc.weight", "last_fc.bias"]
    return fcs + last + ["last_fc_log_std.weight", "last_fc_log_std.bias"], fcs + last


def params_of(meta):
    if meta["kind"] == "goac":
        return goac_params(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["seed"],
                           meta["q_min"], meta["q_max"], pi_init_w=meta["pi_init_w"],
                           q_init_w=meta["q_init_w"])
    return ptrain_params(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["seed"],
                         meta["K"], meta["q_min"], meta["q_max"], pi_init_w=meta["pi_init_w"],
                         q_init_w=meta["q_init_w"])


def make_oracle(meta, dtype=torch.float32, g=None, params=None):
    params = params_of(meta) if params is None else params
    common = dict(q_min=meta["q_min"], q_max=meta["q_max"], discount=meta["discount"],
                  policy_lr=meta["lr"], qf_lr=meta["lr"], tau=meta["tau"],
                  std_soft_update_prob=meta.get("soft"),
                  mean_update=bool(meta.get("mean_update")),
                  train_bias=meta.get("train_bias", True),
                  next_policy=tog.next_policy_of(g) if g is not None else None, dtype=dtype)
    if meta["kind"] == "goac":
        return so.GaussianOACOracle(params, meta["obs_dim"], meta["act_dim"],
                                    delta=meta["delta"], **common)
    return so.ParticleUBOracle(params, meta["obs_dim"], meta["act_dim"], meta["K"],
                               meta["delta_index"], rescale=bool(meta.get("rescale")), **common)


def stats_of(meta, out):
    return tog.goac_stats(out) if meta["kind"] == "goac" else tog.ptrain_stats(meta, out)


def oracle_errors(meta, g, dtype=torch.float32):
    """{key: error} of the oracle's run of the fixture's steps against the
    reference's recorded gradients, post-step parameters and statistics."""
    orc = make_oracle(meta, dtype, g)
    pol_order, q_order = orders(len(meta["hidden"]))
    errs = {}
    for s in range(meta["steps"]):
        b = tog.build_batch(meta, g[f"s{s}/idx"])
        if meta["counts"]:
            b["counts"] = g[f"s{s}/counts"][:, None]
        out = orc.step(b)
        for grp in ("policy", "target_policy", "qf"):
            for pn in (q_order if grp == "qf" else pol_order):
                key = f"s{s}/grad/{grp}/{pn}"
                errs[key] = parity.compare(g, key, out["grads"][grp][pn].numpy())
        for grp, params_ in (("policy", orc.P), ("target_policy", orc.TP), ("qf", orc.Q),
                             ("tf", orc.T)):
            assert list(params_) == (q_order if grp in ("qf", "tf") else pol_order)
            for pn, t in params_.items():
                key = f"s{s}/post/{grp}/{pn}"
                gk = f"s{s}/grad/{grp}/{pn}" if s == 0 and grp != "tf" else None
                errs[key], _ = parity.compare_post(g, key, gk, t.numpy(), meta["lr"])
        errs.update(tog.stat_errors(s, g, stats_of(meta, out)))
    return errs


def det_producers(params):
    """Producers in the reference constructors' call order (policy,
    target_policy, use_target_policy's network; four unused critics, the
    shared-layer critic and its target)."""
    pols = iter([params["policy"], params["target_policy"], params["policy"]])
    qs = iter([params["qf1"]] * 4 + [params["qf1"], params["target_qf1"]])
    return (lambda **k: StateDictModule(next(pols)),
            lambda **k: StateDictModule(next(qs)))


def trainer_for(meta, params=None, **kw):
    """The oac_amd trainer of a fixture's meta (kind 'goac' or 'ptrain')."""
    import oac_amd
    params = params_of(meta) if params is None else params
    pp, qp = det_producers(params)
    soft = meta.get("soft")
    common = dict(action_space=Space(meta["act_dim"]), discount=meta["discount"],
                  reward_scale=1.0, delta=meta["delta"], policy_lr=meta["lr"],
                  qf_lr=meta["lr"], soft_target_tau=meta["tau"], target_update_period=1,
                  q_min=meta["q_min"], q_max=meta["q_max"], share_layers=True,
                  counts=bool(meta.get("counts")), mean_update=bool(meta.get("mean_update")),
                  std_soft_update=soft is not None,
                  std_soft_update_prob=0.0 if soft is None else soft,
                  train_bias=meta.get("train_bias", True),
                  use_target_policy=bool(meta.get("use_target_policy")))
    common.update(kw)
    if meta["kind"] == "goac":
        return oac_amd.GaussianTrainer(pp, qp, n_estimators=2, **common)
    return oac_amd.ParticleTrainer(pp, qp, n_estimators=meta["K"],
                                   rescale_targets_around_mean=bool(meta.get("rescale")),
                                   **common)


def critic_of(tr):
    return tr.qfs[0], tr.tfs[0]


def load_tpn(tr, g):
    """use_target_policy fixtures: the recorded target network's weights."""
    tr.target_policy_network.load_state_dict(
        {k[4:]: torch.as_tensor(np.asarray(v)) for k, v in g.items() if k.startswith("tpn/")})


# ------------------------------------------- mid-training state, own-state oracle
LOG_STD_HEAD = ("last_fc_log_std.weight", "last_fc_log_std.bias")


def det_mid_state(groups, t, seed):
    """fixtures_lib.mid_state for the deterministic-policy trainers: ``groups``
    = {name: parameter dict} (policy, target_policy and each critic).  The
    log-std heads never get a gradient, so torch's Adam keeps no state for them
    (and the step leaves them bit-untouched): their moments stay zero."""
    from fixtures_lib import mid_state
    ms = mid_state(groups, list(groups), t, seed)
    for grp in groups:
        for pn in LOG_STD_HEAD:
            if pn in ms[grp]:
                m, v = ms[grp][pn]
                ms[grp][pn] = (np.zeros_like(m), np.zeros_like(v))
    return ms


def load_mid_state(tr, mods, ms):
    """det_mid_state into a GaussianTrainer / ParticleTrainer (shared or
    separate critics): ``mods`` = {group name: arena module}."""
    from gpu_helpers import module_tensors
    for grp, mod in mods.items():
        m, v = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
        for pn, (mm, vv) in ms[grp].items():
            m[pn].copy_(torch.from_numpy(mm).reshape(m[pn].shape))
            v[pn].copy_(torch.from_numpy(vv).reshape(v[pn].shape))
    tr._n_train_steps_total = ms["t"]
    tr.step_state[0] = ms["t"]


def load_oracle_mid_state(orc, opts, ms):
    """det_mid_state into a CPU oracle: ``opts`` = {group name: its Adam14}."""
    for grp, opt in opts.items():
        for pn, (m, v) in ms[grp].items():
            opt.m[pn].copy_(torch.from_numpy(m).to(opt.m[pn].dtype))
            opt.v[pn].copy_(torch.from_numpy(v).to(opt.v[pn].dtype))
        opt.t = ms["t"]
    orc.n_steps = ms["t"]


def oracle_from_gpu(tr, meta, dtype=torch.float32):
    """The shared-layer oracle holding the GPU trainer's current state
    (parameters, targets, Adam moments and step count)."""
    from gpu_helpers import module_tensors
    torch.cuda.synchronize()
    sd = lambda mod: {k: v.detach().cpu().numpy().copy() for k, v in mod.state_dict().items()}
    qf, tf = critic_of(tr)
    params = dict(policy=sd(tr.policy), target_policy=sd(tr.target_policy), qf1=sd(qf),
                  target_qf1=sd(tf))
    orc = make_oracle(meta, dtype, params=params)
    for opt, mod in ((orc.opt_p, tr.policy), (orc.opt_tp, tr.target_policy), (orc.opt_q, qf)):
        m, v = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
        for k in opt.m:
            opt.m[k].copy_(m[k].detach().cpu())
            opt.v[k].copy_(v[k].detach().cpu())
        opt.t = tr._n_train_steps_total
    orc.n_steps = tr._n_train_steps_total
    return orc


def step_tensors(orc, out, tr=None):
    """{key: float64 array} of a shared-layer step just taken -- every
    gradient, post-step parameter, Adam moment and the Polyak target, whole:
    the oracle's (``tr`` None) or the GPU trainer's."""
    from gpu_helpers import module_tensors
    rec = {}
    cpu = lambda t: t.detach().cpu().double().numpy().copy()
    qf, tf = critic_of(tr) if tr is not None else (None, None)
    for grp, want, opt, mod in (("policy", orc.P, orc.opt_p, getattr(tr, "policy", None)),
                                ("target_policy", orc.TP, orc.opt_tp, getattr(tr, "target_policy", None)),
                                ("qf", orc.Q, orc.opt_q, qf)):
        if tr is not None:
            srcs = (module_tensors(tr, mod, tr.grads), mod.state_dict(),
                    module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v))
        else:
            srcs = (out["grads"][grp], want, opt.m, opt.v)
        for pn in want:
            for what, src in zip(("grad", "post", "adam_m", "adam_v"), srcs):
                rec[f"{what}/{grp}/{pn}"] = cpu(src[pn])
    for pn, t in (tf.state_dict() if tr is not None else orc.T).items():
        rec[f"post/tf/{pn}"] = cpu(t)
    return rec
