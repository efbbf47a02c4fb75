"""CPU restatement of the reference's g-oac and p-oac steps WITHOUT
``--share_layers`` (the trainers' default: gaussian_trainer.py:100-112, 242-271,
344-384; particle_trainer.py:105-114, 186-278, 349-388), in float32 or float64,
from the building blocks of oracle.sac_oracle -- and what the unshared tests
share: the fixtures' parameters, the oracle's errors against a golden, and the
oac_amd trainer of a fixture.

g-oac: two one-output critics, ``q`` (bias = the prior mean, always trained)
and ``std`` (exp'd output, bias = log of the prior std; ``train_bias=False``
freezes its last bias alone), each with its own Adam (``qf_lr`` / ``std_lr``)
and its own MSE loss; the policy ascends q + z std of the post-step critics,
the target policy q alone; Polyak on both.

p-oac: K one-output critics (bias = its initial value).  The K outputs of a
row are sorted; loss i = MSE(sorted_qs[i], targets[i]) is NOT divided by K and
optimizer i steps critic i alone on it, so

    d loss_i / d q_i[r] = 2 (q_i[r] - y_i[r]) / B  where critic i holds sorted
                          rank i in row r, and 0 on every other row

(what loss i sends into the other critics' ``.grad`` is zeroed before it is
ever used).  Targets (counts, std_soft_update, rescale_targets_around_mean)
are the shared step's row math.  The policy ascends the ``delta_index``-th
sorted value of the K post-step critics, the target policy their mean.
"""
import numpy as np
import torch

import parity
import test_oracle_golden as tog
from fixtures_lib import mlp_params
from oracle import sac_oracle as so

FIXTURES = ["goac_us_plain", "goac_us_counts", "goac_us_mean", "goac_us_nobias",
            "ptrain_us_plain", "ptrain_us_counts", "ptrain_us_mean", "ptrain_us_lqg",
            "ptrain_us_nobias_tpn", "ptrain_us_crossed"]
POL_ORDER = ["fc0.weight", "fc0.bias", "last_fc.weight", "last_fc.bias",
             "last_fc_log_std.weight", "last_fc_log_std.bias"]
Q_ORDER = ["fc0.weight", "fc0.bias", "last_fc.weight", "last_fc.bias"]


# ------------------------------------------------------------- parameters
def n_critics(meta):
    return 2 if meta["kind"] == "goac" else meta["K"]


def critic_biases(meta):
    """The last-layer bias each critic is built with (gaussian_trainer.py:70-72,
    101-107; particle_trainer.py:69, 107)."""
    q_min, q_max = meta["q_min"], meta["q_max"]
    if meta["kind"] == "goac":
        return [(q_max + q_min) / 2, np.log((q_max - q_min) / np.sqrt(12))]
    return list(np.linspace(q_min, q_max, meta["K"]))


def params_of(meta):
    """policy, target_policy and the K critics' / target critics' one-output
    networks (fp32).  g-oac: every network drawn on its own; p-oac: each target
    is a copy of its critic (particle_trainer.py:109-111)."""
    Do, Da, hidden = meta["obs_dim"], meta["act_dim"], meta["hidden"]
    rs = np.random.RandomState(meta["seed"])
    pol = mlp_params(rs, Do, hidden, Da, meta["pi_init_w"], log_std_head=True)
    qfs, tfs = [], []
    for b in critic_biases(meta):
        qfs.append(mlp_params(rs, Do + Da, hidden, 1, meta["q_init_w"], last_bias=[b]))
        if meta["kind"] == "goac":
            tfs.append(mlp_params(rs, Do + Da, hidden, 1, meta["q_init_w"], last_bias=[b]))
        else:
            tfs.append({k: v.copy() for k, v in qfs[-1].items()})
    tp = mlp_params(np.random.RandomState(meta["seed"] + 1), Do, hidden, Da, meta["pi_init_w"],
                    log_std_head=True)
    return dict(policy=pol, target_policy=tp, qfs=qfs, tfs=tfs)


# ----------------------------------------------------------------- oracles
class _Unshared(so.GaussianOACOracle):
    """State shared by both unshared oracles: P, TP, NP, the critics ``Qs``
    and targets ``Ts`` (lists of parameter dicts) and one Adam14 per network."""

    def __init__(self, params, obs_dim, act_dim, lrs, frozen, **kw):
        first = dict(policy=params["policy"], target_policy=params["target_policy"],
                     qf1=params["qfs"][0], target_qf1=params["tfs"][0])
        super().__init__(first, obs_dim, act_dim, **kw)
        self.Qs = [so.to_torch_params(p, self.dtype) for p in params["qfs"]]
        self.Ts = [so.to_torch_params(p, self.dtype) for p in params["tfs"]]
        self.opts = [so.Adam14(q, lr) for q, lr in zip(self.Qs, lrs)]
        self.frozen = list(frozen)
        del self.Q, self.T, self.opt_q

    def _inputs(self, batch):
        dt = self.dtype
        return (so._t(batch["observations"], dt), so._t(batch["actions"], dt),
                so._t(batch["rewards"], dt), so._t(batch["terminals"], dt),
                so._t(batch["next_observations"], dt))

    def _critic_grads(self, caches, dqs):
        gs = []
        for k, (c, dq) in enumerate(zip(caches, dqs)):
            g = so.q_param_grads(c, dq, self.Qs[k])
            if self.frozen[k]:                                    # networks.py:59-60
                g["last_fc.bias"] = torch.zeros_like(g["last_fc.bias"])
            gs.append(g)
        return gs

    def _finish(self, gqs, gp, gtp):
        self.opt_p.step(gp)
        self.opt_tp.step(gtp)
        if self.n_steps % self.period == 0:
            for t, q in zip(self.Ts, self.Qs):
                so.polyak(t, q, self.tau)
        self.n_steps += 1
        grads = dict(policy=gp, target_policy=gtp)
        grads.update({f"qf{k}": g for k, g in enumerate(gqs)})
        return grads


class GaussianUnsharedOracle(_Unshared):
    def __init__(self, params, obs_dim, act_dim, qf_lr=3e-4, std_lr=3e-5, train_bias=True, **kw):
        super().__init__(params, obs_dim, act_dim, [qf_lr, std_lr], [False, not train_bias],
                         qf_lr=qf_lr, train_bias=train_bias, **kw)

    def step(self, batch):
        obs, act, rew, term, nobs = self._inputs(batch)
        B = obs.shape[0]
        Q, S = self.Qs
        cq, cs = so.q_forward(obs, act, Q), so.q_forward(obs, act, S)          # :190, :252
        q_preds, std_preds = cq["q"], torch.exp(cs["q"])
        pf2 = so.policy_forward(nobs, self._next_policy(), None, deterministic=True)   # :194-205
        tq0 = so.q_forward(nobs, pf2["a"], self.Ts[0])["q"]                    # :207
        tstd = torch.exp(so.q_forward(nobs, pf2["a"], self.Ts[1])["q"])        # :253
        std_target = (1. - term) * self.discount * tstd                        # :254
        if self.soft is not None:                                              # :256-259
            std_target = self.soft * std_target + (1 - self.soft) * std_preds
        if batch.get("counts") is not None:                                    # :261-265
            factor = (so._t(batch["counts"], self.dtype).reshape(B, 1) == 0).to(self.dtype)
            std_target = std_target * factor + (1 - factor) * std_preds
        q_target = self.reward_scale * rew + (1. - term) * self.discount * tq0   # :244-245
        std_target = torch.clamp(std_target, 0, self.std_init)                 # :267
        gqs = self._critic_grads(
            [cq, cs], [2.0 * (q_preds - q_target) / B,
                       2.0 * (std_preds - std_target) / B * std_preds])        # exp backward
        pf = so.policy_forward(obs, self.P, None, deterministic=True)          # :334 (pre-step)
        tpf = so.policy_forward(obs, self.TP, None, deterministic=True)        # :361
        for opt, g in zip(self.opts, gqs):                                     # :249, :271
            opt.step(g)
        nq, ns = so.q_forward(obs, pf["a"], Q), so.q_forward(obs, pf["a"], S)  # :344-349
        stds = torch.exp(ns["q"])
        ub = nq["q"] + self.z * stds                                           # :350
        g0 = -torch.ones_like(ub) / B
        da = (so.q_input_grad(nq, g0, Q) + so.q_input_grad(ns, g0 * self.z * stds, S))[:, self.Do:]
        gp = so.det_policy_backward(pf, self.P, da)
        ct = so.q_forward(obs, tpf["a"], Q)                                    # :365
        gtp = so.det_policy_backward(tpf, self.TP, so.q_input_grad(ct, g0, Q)[:, self.Do:])
        grads = self._finish(gqs, gp, gtp)
        self.last = dict(grads=grads, q_loss=((q_preds - q_target) ** 2).mean(),
                         std_loss=((std_preds - std_target) ** 2).mean(), q_preds=q_preds,
                         std_preds=std_preds, q_target=q_target, std_target=std_target,
                         upper_bound=ub, target_head=tpf)
        return self.last


def min_rank_gap(qs):
    """Smallest gap between adjacent sorted values of a row of ``qs`` [K, B],
    relative to the row's spread (seed condition b of the p-oac fixtures)."""
    s = torch.sort(qs.double(), dim=0)[0]
    spread = (s[-1] - s[0]).clamp_min(1e-300)
    return float(((s[1:] - s[:-1]).min(dim=0)[0] / spread).min())


class ParticleUnsharedOracle(_Unshared):
    def __init__(self, params, obs_dim, act_dim, K, delta_index, q_min=0.0, q_max=100.0,
                 qf_lr=1e-3, rescale=False, train_bias=True, **kw):
        super().__init__(params, obs_dim, act_dim, [qf_lr] * K, [not train_bias] * K,
                         q_min=q_min, q_max=q_max, qf_lr=qf_lr, train_bias=train_bias, **kw)
        self.K, self.delta_index = K, delta_index
        self.spread = (q_max - q_min) if rescale else None

    def _stack(self, obs, act, nets):
        cs = [so.q_forward(obs, act, p) for p in nets]
        return cs, torch.stack([c["q"][:, 0] for c in cs], dim=0)              # [K, B]

    def step(self, batch):
        obs, act, rew, term, nobs = self._inputs(batch)
        B, K = obs.shape[0], self.K
        cs, qs = self._stack(obs, act, self.Qs)                                # :186-190
        sorted_qs, idx = torch.sort(qs, dim=0)                                 # :193
        pf2 = so.policy_forward(nobs, self._next_policy(), None, deterministic=True)   # :194-206
        _, tq = self._stack(nobs, pf2["a"], self.Ts)                           # :210-211
        tq_sorted, _ = torch.sort(tq, dim=0)                                   # :214
        y = self.reward_scale * rew.t() + (1. - term.t()) * self.discount * tq_sorted   # :218-219
        if self.soft is not None:                                              # :221-231
            y = self.soft * y + (1 - self.soft) * (sorted_qs - torch.mean(sorted_qs, dim=0)
                                                   + torch.mean(y, dim=0))
        if batch.get("counts") is not None:                                    # :233-238
            factor = (so._t(batch["counts"], self.dtype).reshape(1, B) == 0).to(self.dtype)
            y = y * factor + (1 - factor) * (sorted_qs - torch.mean(sorted_qs, dim=0)
                                             + torch.mean(y, dim=0))
        if self.spread is not None:                                            # :253-260
            q_range = y[-1] - y[0]
            factor = torch.ones_like(q_range)
            factor[q_range > self.spread] = 0
            q_mean = torch.mean(y, dim=0)
            y = factor * y + (1 - factor) * ((y - q_mean) * (self.spread / (q_range + 1e-6))
                                             + q_mean)
        losses = ((sorted_qs - y) ** 2).mean(dim=1)                            # :273
        # loss i reaches critic i through the rows where it holds rank i     :276-278
        own = idx == torch.arange(K)[:, None]
        dq = 2.0 * (sorted_qs - y) / B * own.to(self.dtype)
        gqs = self._critic_grads(cs, [dq[k][:, None] for k in range(K)])
        pf = so.policy_forward(obs, self.P, None, deterministic=True)          # :340 (pre-step)
        tpf = so.policy_forward(obs, self.TP, None, deterministic=True)        # :367
        for opt, g in zip(self.opts, gqs):
            opt.step(g)
        cn, pq = self._stack(obs, pf["a"], self.Qs)                            # :349-351
        sq, sidx = torch.sort(pq, dim=0)                                       # :354
        ub = sq[self.delta_index]                                              # :355
        g0 = -torch.ones_like(ub) / B
        gsel = torch.zeros_like(pq).scatter_(0, sidx[self.delta_index:self.delta_index + 1],
                                             g0[None])
        da = sum(so.q_input_grad(cn[k], gsel[k][:, None], self.Qs[k]) for k in range(K))
        gp = so.det_policy_backward(pf, self.P, da[:, self.Do:])
        ct, tpq = self._stack(obs, tpf["a"], self.Qs)                          # :371-375
        dat = sum(so.q_input_grad(ct[k], (g0 / K)[:, None], self.Qs[k]) for k in range(K))
        gtp = so.det_policy_backward(tpf, self.TP, dat[:, self.Do:])
        grads = self._finish(gqs, gp, gtp)
        self.last = dict(grads=grads, qf_losses=losses, qf_loss=losses.sum(),   # (:275: not / K)
                         sorted_qs=sorted_qs, y=y, tq=tq, upper_bound=ub, target_head=tpf,
                         out_of_rank=float((~own).double().mean()),
                         min_gap=min(min_rank_gap(qs), min_rank_gap(tq), min_rank_gap(pq)))
        return self.last


def make_oracle(meta, dtype=torch.float32, g=None, params=None):
    params = params_of(meta) if params is None else params
    common = dict(q_min=meta["q_min"], q_max=meta["q_max"], discount=meta["discount"],
                  policy_lr=meta["lr"], qf_lr=meta["lr"], tau=meta["tau"],
                  std_soft_update_prob=meta.get("soft"),
                  mean_update=bool(meta.get("mean_update")),
                  train_bias=meta.get("train_bias", True),
                  next_policy=tog.next_policy_of(g) if g is not None else None, dtype=dtype)
    if meta["kind"] == "goac":
        return GaussianUnsharedOracle(params, meta["obs_dim"], meta["act_dim"],
                                      delta=meta["delta"], std_lr=meta["std_lr"], **common)
    return ParticleUnsharedOracle(params, meta["obs_dim"], meta["act_dim"], meta["K"],
                                  meta["delta_index"], rescale=bool(meta.get("rescale")), **common)


def stats_of(meta, out):
    return tog.goac_stats(out) if meta["kind"] == "goac" else tog.ptrain_stats(meta, out)


def critic_lr(meta, k):
    return meta["std_lr"] if (meta["kind"] == "goac" and k == 1) else meta["lr"]


def batch_of(meta, g, s):
    b = tog.build_batch(meta, g[f"s{s}/idx"])
    if meta["counts"]:
        b["counts"] = g[f"s{s}/counts"][:, None]
    return b


def oracle_errors(meta, g, dtype=torch.float32, extras=None):
    """{key: error} of the oracle's run of the fixture's steps against the
    reference's recorded gradients, post-step parameters, Adam moments and
    statistics -- every critic, every element.  ``extras`` (a dict) receives the
    run's smallest rank gap and the out-of-rank share of step 0."""
    orc = make_oracle(meta, dtype, g)
    K = n_critics(meta)
    errs = {}
    for s in range(meta["steps"]):
        out = orc.step(batch_of(meta, g, s))
        if extras is not None and meta["kind"] == "ptrain":
            extras["min_gap"] = min(extras.get("min_gap", np.inf), out["min_gap"])
            extras.setdefault("out_of_rank", out["out_of_rank"])
        groups = [("policy", orc.P, POL_ORDER, meta["lr"]),
                  ("target_policy", orc.TP, POL_ORDER, meta["lr"])]
        groups += [(f"qf{k}", orc.Qs[k], Q_ORDER, critic_lr(meta, k)) for k in range(K)]
        for grp, params_, order, lr in groups:
            assert list(params_) == order
            for pn in order:
                key = f"s{s}/grad/{grp}/{pn}"
                errs[key] = parity.compare(g, key, out["grads"][grp][pn].numpy())
                key = f"s{s}/post/{grp}/{pn}"
                gk = f"s{s}/grad/{grp}/{pn}" if s == 0 else None
                errs[key], _ = parity.compare_post(g, key, gk, params_[pn].numpy(), lr)
        for k in range(K):
            for pn in Q_ORDER:
                key = f"s{s}/post/tf{k}/{pn}"
                errs[key] = parity.compare(g, key, orc.Ts[k][pn].numpy())
                for nm, mom in (("m", orc.opts[k].m), ("v", orc.opts[k].v)):
                    key = f"s{s}/adam_{nm}/qf{k}/{pn}"
                    errs[key] = parity.compare(g, key, mom[pn].numpy())
        errs.update(tog.stat_errors(s, g, stats_of(meta, out)))
    return errs


# ------------------------------------------------------- the oac_amd trainer
def producers(params, kind):
    """Producers in the reference constructors' call order: policy,
    target_policy, use_target_policy's network; four unused critics, then q,
    q_target, std, std_target (g-oac) or critic, target per particle (p-oac)."""
    from gpu_helpers import StateDictModule
    pols = iter([params["policy"], params["target_policy"], params["policy"]])
    if kind == "goac":
        seq = [params["qfs"][0], params["tfs"][0], params["qfs"][1], params["tfs"][1]]
    else:
        seq = [p for pair in zip(params["qfs"], params["tfs"]) for p in pair]
    qs = iter([params["qfs"][0]] * 4 + seq)
    calls = []

    def q_producer(**kw):
        calls.append(kw)
        return StateDictModule(next(qs))
    q_producer.calls = calls
    return (lambda **k: StateDictModule(next(pols))), q_producer


def trainer_for(meta, params=None, **kw):
    """The oac_amd trainer of a fixture's meta, share_layers=False."""
    import oac_amd
    from gpu_helpers import Space
    params = params_of(meta) if params is None else params
    pp, qp = producers(params, meta["kind"])
    soft = meta.get("soft")
    common = dict(action_space=Space(meta["act_dim"]), discount=meta["discount"],
                  reward_scale=1.0, delta=meta["delta"], policy_lr=meta["lr"],
                  qf_lr=meta["lr"], soft_target_tau=meta["tau"], target_update_period=1,
                  q_min=meta["q_min"], q_max=meta["q_max"], share_layers=False,
                  counts=bool(meta.get("counts")), mean_update=bool(meta.get("mean_update")),
                  std_soft_update=soft is not None,
                  std_soft_update_prob=0.0 if soft is None else soft,
                  train_bias=meta.get("train_bias", True),
                  use_target_policy=bool(meta.get("use_target_policy")))
    common.update(kw)
    if meta["kind"] == "goac":
        tr = oac_amd.GaussianTrainer(pp, qp, n_estimators=2, std_lr=meta["std_lr"], **common)
    else:
        tr = oac_amd.ParticleTrainer(pp, qp, n_estimators=meta["K"],
                                     rescale_targets_around_mean=bool(meta.get("rescale")),
                                     **common)
    tr.q_producer_calls = qp.calls
    return tr


# ------------------------------------------------- oracle from the GPU's state
def _np_sd(mod):
    return {k: v.detach().cpu().numpy().copy() for k, v in mod.state_dict().items()}


def _load_adam(opt, tr, mod):
    from gpu_helpers import module_tensors
    m, v = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
    for k in opt.m:
        opt.m[k].copy_(m[k].detach().cpu())
        opt.v[k].copy_(v[k].detach().cpu())
    opt.t = tr._n_train_steps_total


def oracle_from_gpu(tr, meta, g=None, dtype=torch.float32):
    """The oracle (fp32 unless ``dtype`` says otherwise) holding the GPU
    trainer's current state (teacher forcing)."""
    torch.cuda.synchronize()
    params = dict(policy=_np_sd(tr.policy), target_policy=_np_sd(tr.target_policy),
                  qfs=[_np_sd(q) for q in tr.qfs], tfs=[_np_sd(t) for t in tr.tfs])
    orc = make_oracle(meta, dtype=dtype, g=g, params=params)
    _load_adam(orc.opt_p, tr, tr.policy)
    _load_adam(orc.opt_tp, tr, tr.target_policy)
    for opt, q in zip(orc.opts, tr.qfs):
        _load_adam(opt, tr, q)
    orc.n_steps = tr._n_train_steps_total
    return orc


def _groups(tr, orc, meta):
    K = n_critics(meta)
    gs = [("policy", tr.policy, orc.P, orc.opt_p, meta["lr"]),
          ("target_policy", tr.target_policy, orc.TP, orc.opt_tp, meta["lr"])]
    return gs + [(f"qf{k}", tr.qfs[k], orc.Qs[k], orc.opts[k], critic_lr(meta, k))
                 for k in range(K)]


def step_tensors(orc, out, meta, tr=None):
    """{key: array} of a step just taken, keyed as step_errors_against_oracle
    keys its errors: the oracle's (``tr`` None) or the GPU trainer's.  The K
    critics' last biases are gathered into the [K] vector 'qf*'."""
    from gpu_helpers import module_tensors
    rec, stacked = {}, {}
    K = n_critics(meta)
    groups = [("policy", orc.P, orc.opt_p), ("target_policy", orc.TP, orc.opt_tp)]
    groups += [(f"qf{k}", orc.Qs[k], orc.opts[k]) for k in range(K)]
    for grp, want, opt in groups:
        if tr is not None:
            mod = tr.qfs[int(grp[2:])] if grp.startswith("qf") else getattr(tr, grp)
            gv = module_tensors(tr, mod, tr.grads)
            mv, vv = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
            sd = mod.state_dict()
            get = lambda d, pn: d[pn].detach().cpu().double().numpy()
            vals = lambda pn: (get(gv, pn), get(sd, pn), get(mv, pn), get(vv, pn))
        else:
            get = lambda d, pn: d[pn].double().numpy().copy()
            vals = lambda pn: (get(out["grads"][grp], pn), get(want, pn), get(opt.m, pn), get(opt.v, pn))
        for pn in want:
            for what, v in zip(("grad", "post", "adam_m", "adam_v"), vals(pn)):
                if grp.startswith("qf") and pn == "last_fc.bias":
                    stacked.setdefault(what, []).append(float(v.reshape(-1)[0]))
                else:
                    rec[f"{what}/{grp}/{pn}"] = v
    for what, v in stacked.items():
        rec[f"{what}/qf*/last_fc.bias"] = np.array(v)
    for k in range(K):
        src = tr.tfs[k].state_dict() if tr is not None else orc.Ts[k]
        for pn, t in src.items():
            rec[f"post/tf{k}/{pn}"] = t.detach().cpu().double().numpy()
    return rec


def step_errors_against_oracle(tr, orc, out, meta):
    """{key: error} of the GPU step just taken against the oracle's step from
    the same pre-step state: every gradient, post-step parameter and Adam
    moment of every network, and every target critic, norm-relative per tensor.

    A critic's last_fc.bias is ONE number, and its gradient sum_r dq[r] a sum of
    B terms of both signs: two correct fp32 sums differ by ~B eps sum|dq[r]|,
    which relative to the sum itself is unbounded (cancellation) -- a [K]
    vector's norm averages that out, a scalar's does not.  The K critics'
    biases (gradient, Adam moments, post-step value) are therefore compared as
    the [K] vector they form in the stacked block (key 'qf*'), which is also
    what the shared-layer step's last_fc.bias is."""
    from gpu_helpers import module_tensors
    torch.cuda.synchronize()
    errs = {}
    stacked = {}
    for grp, mod, want, opt, lr in _groups(tr, orc, meta):
        gv = module_tensors(tr, mod, tr.grads)
        mv, vv = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
        sd = mod.state_dict()
        for pn in want:
            gref = out["grads"][grp][pn].numpy()
            if grp.startswith("qf") and pn == "last_fc.bias":
                for what, got, ref in (("grad", gv[pn], gref), ("post", sd[pn], want[pn].numpy()),
                                       ("adam_m", mv[pn], opt.m[pn].numpy()),
                                       ("adam_v", vv[pn], opt.v[pn].numpy())):
                    a, b = stacked.setdefault(what, ([], []))
                    a.append(float(got.cpu().reshape(-1)[0]))
                    b.append(float(np.asarray(ref).reshape(-1)[0]))
                continue
            errs[f"grad/{grp}/{pn}"] = parity.rel_err(gv[pn].cpu().numpy(), gref)
            errs[f"post/{grp}/{pn}"], _ = parity.compare_post(
                {"p": want[pn].numpy(), "g": gref}, "p", "g", sd[pn].cpu().numpy(), lr)
            errs[f"adam_m/{grp}/{pn}"] = parity.rel_err(mv[pn].cpu().numpy(), opt.m[pn].numpy())
            errs[f"adam_v/{grp}/{pn}"] = parity.rel_err(vv[pn].cpu().numpy(), opt.v[pn].numpy())
    lr = meta["lr"]
    for what, (got, ref) in stacked.items():
        if what == "post":   # (outside Adam's sign band of the gradient vector, as compare_post)
            errs["post/qf*/last_fc.bias"], _ = parity.compare_post(
                {"p": np.array(ref), "g": np.array(stacked["grad"][1])}, "p", "g", np.array(got), lr)
        else:
            errs[f"{what}/qf*/last_fc.bias"] = parity.rel_err(got, ref)
    for k, tf in enumerate(tr.tfs):
        for pn, t in tf.state_dict().items():
            errs[f"post/tf{k}/{pn}"] = parity.rel_err(t.cpu().numpy(), orc.Ts[k][pn].numpy())
    return errs
