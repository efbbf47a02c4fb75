"""CPU restatement of the reference's p-oac step with a policy ENSEMBLE
(``ParticleTrainer(ensemble=True, n_policies=P)`` without ``--share_layers``,
deterministic policies, one hidden layer: particle_trainer.py:115-137, 203-206,
321-338; ``EnsemblePolicy``, trainer/policies.py:546-647), in float32 or
float64, from the building blocks of oracle.sac_oracle and
tests/unshared_oracle.py -- and what the ensemble tests share: the fixtures'
parameters, the oracle's errors against a golden, the acting oracle, the sweep
cases and the oac_amd trainer of a fixture.

Per step: the K critics' sorted-particle targets as without the ensemble, but
the next action of a row is the proposal a'_p = tanh(mean_p(next_obs)) with the
largest UB_p = sort_k(q_k(next_obs, a'_p))[delta_index] under the K ONLINE,
pre-step critics (the first maximum wins; with ``mean_update`` the target policy
acts and nothing is selected); then policy p alone ascends mean(UB_p) of the
post-step critics on (obs, tanh(mean_p(obs))), one Adam per policy; the target
policy ascends the critics' mean.  'Policy Loss' is the LAST policy's mean(UB).
"""
import numpy as np
import torch

import parity
import test_oracle_golden as tog
import unshared_oracle as uo
from fixtures_lib import mlp_params, synthetic_transitions
from oracle import sac_oracle as so

FIXTURES = ["ens_plain", "ens_counts", "ens_mean", "ens_ragged"]
POL_ORDER, Q_ORDER = uo.POL_ORDER, uo.Q_ORDER
MIN_GAP = 1e-4


# ------------------------------------------------------------- parameters
def params_of(meta):
    """target_policy and the K critics / targets as the unshared p-oac fixtures
    build them, plus the P policies: each drawn on a stream of its own, its mean
    head's bias arctanh(initial_actions[p]) in every action dimension
    (policies.py:224-225, 569) -- ``meta['initial_actions']`` holds what the
    trainer's constructor passes (the reference's own values in a golden)."""
    base = uo.params_of(meta)
    Do, Da, hidden = meta["obs_dim"], meta["act_dim"], meta["hidden"]
    pols = []
    for p in range(meta["P"]):
        rs = np.random.RandomState(meta["seed"] + 10 + p)
        pol = mlp_params(rs, Do, hidden, Da, meta["pi_init_w"], log_std_head=True)
        pol["last_fc.bias"] = np.full(Da, np.arctanh(meta["initial_actions"][p]), np.float32)
        pols.append(pol)
    base["policies"] = pols
    base["policy"] = pols[0]
    return base


def first_max(ubs):
    """argmax over dim 0 of ubs [P, B] with a strict '>' scan: the first maximum."""
    best, sel = ubs[0].clone(), torch.zeros(ubs.shape[1], dtype=torch.long)
    for p in range(1, ubs.shape[0]):
        m = ubs[p] > best
        sel[m] = p
        best[m] = ubs[p][m]
    return sel


def selection_gap(ubs):
    """Smallest (best - second best) UB_p of a row relative to the row's spread
    of UB_p (seed condition c); inf for one policy."""
    if ubs.shape[0] < 2:
        return float("inf")
    s = torch.sort(ubs.double(), dim=0)[0]
    spread = (s[-1] - s[0]).clamp_min(1e-300)
    return float(((s[-1] - s[-2]) / spread).min())


# ----------------------------------------------------------------- oracle
class EnsembleOracle(uo.ParticleUnsharedOracle):
    def __init__(self, params, obs_dim, act_dim, K, delta_index, policy_lr=1e-3, **kw):
        super().__init__(params, obs_dim, act_dim, K, delta_index, policy_lr=policy_lr, **kw)
        self.Ps = [so.to_torch_params(p, self.dtype) for p in params["policies"]]
        self.opt_ps = [so.Adam14(p, policy_lr) for p in self.Ps]
        del self.P, self.opt_p

    def upper_bound(self, obs, act, nets):
        """(UB [B], the stacked values [K, B], the critics' caches)."""
        cs, pq = self._stack(obs, act, nets)
        return torch.sort(pq, dim=0)[0][self.delta_index], pq, cs

    def step(self, batch):
        obs, act, rew, term, nobs = self._inputs(batch)
        B, K, di = obs.shape[0], self.K, self.delta_index
        cs, qs = self._stack(obs, act, self.Qs)                                # :186-190
        sorted_qs, idx = torch.sort(qs, dim=0)                                 # :193
        gaps = [uo.min_rank_gap(qs)]
        sel, ub_next, sel_gap = None, None, float("inf")
        if self.mean_update:                                                   # :194-197
            a2 = so.policy_forward(nobs, self.TP, None, deterministic=True)["a"]
        else:                                                                  # :203-206 -> policies.py:596-604
            props = [so.policy_forward(nobs, P, None, deterministic=True)["a"] for P in self.Ps]
            ubs = []
            for a in props:                                # approximator.predict: the ONLINE critics
                ub, pq, _ = self.upper_bound(nobs, a, self.Qs)
                gaps.append(uo.min_rank_gap(pq))
                ubs.append(ub)
            ub_next = torch.stack(ubs, dim=0)                                  # [P, B]
            sel = first_max(ub_next)
            sel_gap = selection_gap(ub_next)
            a2 = torch.stack(props, dim=0)[sel, torch.arange(B)]
        _, tq = self._stack(nobs, a2, self.Ts)                                 # :210-211
        gaps.append(uo.min_rank_gap(tq))
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
        own = idx == torch.arange(K)[:, None]                                  # :276-278
        dq = 2.0 * (sorted_qs - y) / B * own.to(self.dtype)
        gqs = self._critic_grads(cs, [dq[k][:, None] for k in range(K)])
        pfs = [so.policy_forward(obs, P, None, deterministic=True) for P in self.Ps]   # pre-step
        tpf = so.policy_forward(obs, self.TP, None, deterministic=True)        # :367
        for opt, g in zip(self.opts, gqs):
            opt.step(g)
        g0 = -torch.ones(B, dtype=self.dtype) / B
        gps, ubs1 = [], []
        for P, pf in zip(self.Ps, pfs):                                        # :322-338
            cn, pq = self._stack(obs, pf["a"], self.Qs)
            gaps.append(uo.min_rank_gap(pq))
            sq, sidx = torch.sort(pq, dim=0)
            ubs1.append(sq[di])
            gsel = torch.zeros_like(pq).scatter_(0, sidx[di:di + 1], g0[None])
            da = sum(so.q_input_grad(cn[k], gsel[k][:, None], self.Qs[k]) for k in range(K))
            gps.append(so.det_policy_backward(pf, P, da[:, self.Do:]))
        ct, _ = self._stack(obs, tpf["a"], self.Qs)                            # :371-375
        dat = sum(so.q_input_grad(ct[k], (g0 / K)[:, None], self.Qs[k]) for k in range(K))
        gtp = so.det_policy_backward(tpf, self.TP, dat[:, self.Do:])
        for opt, g in zip(self.opt_ps, gps):
            opt.step(g)
        self.opt_tp.step(gtp)
        if self.n_steps % self.period == 0:
            for t, q in zip(self.Ts, self.Qs):
                so.polyak(t, q, self.tau)
        self.n_steps += 1
        grads = dict(target_policy=gtp)
        grads.update({f"policy{p}": g for p, g in enumerate(gps)})
        grads.update({f"qf{k}": g for k, g in enumerate(gqs)})
        self.last = dict(grads=grads, qf_losses=losses, qf_loss=losses.sum(), sorted_qs=sorted_qs,
                         y=y, tq=tq, upper_bound=ubs1[-1], upper_bounds=torch.stack(ubs1, dim=0),
                         target_head=tpf, sel=sel, ub_next=ub_next, sel_gap=sel_gap,
                         obs_actions=torch.stack([pf["a"] for pf in pfs], dim=0),
                         out_of_rank=float((~own).double().mean()), min_gap=min(gaps))
        return self.last

    # ------------------------------------------------------------- acting
    def act(self, obs, noise=None):
        """EnsemblePolicy.forward / get_action (policies.py:576-631) on obs
        [N, Do]: proposals [P, N, Da], UB [P, N], the first-maximum index [N]
        and the chosen policy's six ``forward`` outputs.  ``noise`` [N, P, Da]:
        the sampled call (log_prob is then the summed [N, 1] term)."""
        x = so._t(obs, self.dtype)
        N = x.shape[0]
        pfs = []
        for p, P in enumerate(self.Ps):
            eps = None if noise is None else so._t(np.asarray(noise)[:, p], self.dtype)
            pfs.append(so.policy_forward(x, P, eps, deterministic=noise is None))
        ubs = torch.stack([self.upper_bound(x, pf["a"], self.Qs)[0] for pf in pfs], dim=0)
        sel = first_max(ubs)
        pick = lambda key: torch.stack([pf[key] for pf in pfs], dim=0)[sel, torch.arange(N)]
        six = dict(action=pick("a"), mean=pick("mean"), log_std=pick("log_std"), std=pick("std"))
        if noise is None:
            six["log_prob"], six["pre_tanh"] = torch.zeros_like(six["action"]), six["mean"]
        else:
            six["log_prob"], six["pre_tanh"] = pick("logp"), pick("z")
        return dict(proposals=torch.stack([pf["a"] for pf in pfs], dim=0), ub=ubs, sel=sel,
                    sel_gap=selection_gap(ubs), **six)


def make_oracle(meta, dtype=torch.float32, params=None):
    params = params_of(meta) if params is None else params
    return EnsembleOracle(params, meta["obs_dim"], meta["act_dim"], meta["K"], meta["delta_index"],
                          q_min=meta["q_min"], q_max=meta["q_max"], discount=meta["discount"],
                          policy_lr=meta["lr"], qf_lr=meta["lr"], tau=meta["tau"],
                          std_soft_update_prob=meta.get("soft"),
                          mean_update=bool(meta.get("mean_update")),
                          train_bias=meta.get("train_bias", True),
                          rescale=bool(meta.get("rescale")), dtype=dtype)


def batch_of(meta, g, s):
    return uo.batch_of(meta, g, s)


def groups_of(orc, meta):
    """(name, parameters, Adam, order, lr) of every network with an optimizer."""
    gs = [(f"policy{p}", orc.Ps[p], orc.opt_ps[p], POL_ORDER) for p in range(meta["P"])]
    gs.append(("target_policy", orc.TP, orc.opt_tp, POL_ORDER))
    gs += [(f"qf{k}", orc.Qs[k], orc.opts[k], Q_ORDER) for k in range(meta["K"])]
    return gs


def oracle_errors(meta, g, dtype=torch.float32, extras=None):
    """{key: error} of the oracle's run of the fixture's steps against the
    reference's recording -- every policy's and critic's gradient, post-step
    parameters and Adam moments, every target critic, the target critics'
    values on the chosen next actions and the statistics, every element; the
    chosen indices must be EQUAL.  ``extras`` receives the margins: the
    smallest rank gap, the smallest selection gap, and step 0's share of rows
    per chosen policy."""
    orc = make_oracle(meta, dtype)
    errs = {}
    for s in range(meta["steps"]):
        out = orc.step(batch_of(meta, g, s))
        if extras is not None:
            extras["min_gap"] = min(extras.get("min_gap", np.inf), out["min_gap"])
            extras["sel_gap"] = min(extras.get("sel_gap", np.inf), out["sel_gap"])
            if s == 0 and out["sel"] is not None:
                extras["chosen_share"] = (np.bincount(out["sel"].numpy(), minlength=meta["P"])
                                          / float(meta["B"])).tolist()
        if out["sel"] is not None:
            assert np.array_equal(out["sel"].numpy(), g[f"s{s}/sel"]), (s, "chosen indices differ")
        else:
            assert f"s{s}/sel" not in g
        errs[f"s{s}/tq"] = parity.compare(g, f"s{s}/tq", out["tq"].numpy())
        for grp, params_, opt, order in groups_of(orc, meta):
            assert list(params_) == order
            for pn in order:
                key = f"s{s}/grad/{grp}/{pn}"
                errs[key] = parity.compare(g, key, out["grads"][grp][pn].numpy())
                key = f"s{s}/post/{grp}/{pn}"
                gk = f"s{s}/grad/{grp}/{pn}" if s == 0 else None
                errs[key], _ = parity.compare_post(g, key, gk, params_[pn].numpy(), meta["lr"])
                for nm, mom in (("m", opt.m), ("v", opt.v)):
                    key = f"s{s}/adam_{nm}/{grp}/{pn}"
                    errs[key] = parity.compare(g, key, mom[pn].numpy())
        for k in range(meta["K"]):
            for pn in Q_ORDER:
                key = f"s{s}/post/tf{k}/{pn}"
                errs[key] = parity.compare(g, key, orc.Ts[k][pn].numpy())
        errs.update(tog.stat_errors(s, g, tog.ptrain_stats(meta, out)))
    return errs


# ------------------------------------------------------- the oac_amd trainer
class Space:
    """action_space of the constructor: shape, low and high."""

    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, np.float32), np.ones(n, np.float32)


class EnsembleModules:
    """What policy_producer(ensemble=True) returns: any object with ``.policies``."""

    def __init__(self, sds):
        from gpu_helpers import StateDictModule
        self.policies = [StateDictModule(sd) for sd in sds]


def producers(params):
    """Producers in the reference constructor's call order: SACTrainer's policy
    (discarded), the ensemble, target_policy; four unused critics, then critic
    and target per particle.  ``policy_producer.calls`` records the keyword
    arguments of each call."""
    from gpu_helpers import StateDictModule
    pols = iter([params["policies"][0], params["target_policy"]])
    qs = iter([params["qfs"][0]] * 4 + [p for pair in zip(params["qfs"], params["tfs"]) for p in pair])
    calls = []

    def policy_producer(**kw):
        calls.append(kw)
        if kw.get("ensemble"):
            return EnsembleModules(params["policies"])
        return StateDictModule(next(pols))
    policy_producer.calls = calls
    return policy_producer, (lambda **kw: StateDictModule(next(qs)))


def trainer_for(meta, params=None, **kw):
    """The oac_amd ParticleTrainer(ensemble=True) of a fixture's meta."""
    import oac_amd
    params = params_of(meta) if params is None else params
    pp, qp = producers(params)
    soft = meta.get("soft")
    common = dict(n_estimators=meta["K"], action_space=Space(meta["act_dim"]),
                  discount=meta["discount"], reward_scale=1.0, delta=meta["delta"],
                  policy_lr=meta["lr"], qf_lr=meta["lr"], soft_target_tau=meta["tau"],
                  target_update_period=1, q_min=meta["q_min"], q_max=meta["q_max"],
                  share_layers=False, ensemble=True, n_policies=meta["P"],
                  counts=bool(meta.get("counts")), mean_update=bool(meta.get("mean_update")),
                  std_soft_update=soft is not None,
                  std_soft_update_prob=0.0 if soft is None else soft,
                  train_bias=meta.get("train_bias", True),
                  rescale_targets_around_mean=bool(meta.get("rescale")))
    common.update(kw)
    tr = oac_amd.ParticleTrainer(pp, qp, **common)
    tr.policy_producer_calls = pp.calls
    return tr


def _np_sd(mod):
    return {k: v.detach().cpu().numpy().copy() for k, v in mod.state_dict().items()}


def oracle_from_gpu(tr, meta, dtype=torch.float32):
    """The oracle holding the GPU trainer's current state (teacher forcing)."""
    torch.cuda.synchronize()
    params = dict(policies=[_np_sd(p) for p in tr.policy.policies],
                  target_policy=_np_sd(tr.target_policy),
                  qfs=[_np_sd(q) for q in tr.qfs], tfs=[_np_sd(t) for t in tr.tfs])
    params["policy"] = params["policies"][0]
    orc = make_oracle(meta, dtype=dtype, params=params)
    for opt, mod in zip(orc.opt_ps, tr.policy.policies):
        uo._load_adam(opt, tr, mod)
    uo._load_adam(orc.opt_tp, tr, tr.target_policy)
    for opt, q in zip(orc.opts, tr.qfs):
        uo._load_adam(opt, tr, q)
    orc.n_steps = tr._n_train_steps_total
    return orc


def gpu_module(tr, grp):
    if grp == "target_policy":
        return tr.target_policy
    return tr.qfs[int(grp[2:])] if grp.startswith("qf") else tr.policy.policies[int(grp[6:])]


def step_errors_against_oracle(tr, orc, out, meta):
    """{key: error} of the GPU step just taken against the oracle's step from
    the same pre-step state: every gradient, post-step parameter and Adam
    moment of every network and every target critic, norm-relative per tensor,
    nothing left out.  The K critics' one-number last biases are compared as
    the [K] vector they form (key 'qf*', as tests/unshared_oracle.py explains);
    so are, for the same reason, the P policies' [Da] mean-head biases when
    Da == 1 (key 'policy*')."""
    from gpu_helpers import module_tensors
    torch.cuda.synchronize()
    errs, stacked = {}, {}
    lr = meta["lr"]
    for grp, want, opt, order in groups_of(orc, meta):
        mod = gpu_module(tr, grp)
        gv = module_tensors(tr, mod, tr.grads)
        mv, vv = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
        sd = mod.state_dict()
        for pn in want:
            gref = out["grads"][grp][pn].numpy()
            star = ("qf*" if grp.startswith("qf") and pn == "last_fc.bias" else
                    "policy*" if grp.startswith("policy") and pn == "last_fc.bias"
                    and meta["act_dim"] == 1 else None)
            if star:
                for what, got, ref in (("grad", gv[pn], gref), ("post", sd[pn], want[pn].numpy()),
                                       ("adam_m", mv[pn], opt.m[pn].numpy()),
                                       ("adam_v", vv[pn], opt.v[pn].numpy())):
                    a, b = stacked.setdefault((what, star), ([], []))
                    a.append(float(got.cpu().reshape(-1)[0]))
                    b.append(float(np.asarray(ref).reshape(-1)[0]))
                continue
            errs[f"grad/{grp}/{pn}"] = parity.rel_err(gv[pn].cpu().numpy(), gref)
            errs[f"post/{grp}/{pn}"], _ = parity.compare_post(
                {"p": want[pn].numpy(), "g": gref}, "p", "g", sd[pn].cpu().numpy(), lr)
            errs[f"adam_m/{grp}/{pn}"] = parity.rel_err(mv[pn].cpu().numpy(), opt.m[pn].numpy())
            errs[f"adam_v/{grp}/{pn}"] = parity.rel_err(vv[pn].cpu().numpy(), opt.v[pn].numpy())
    for (what, star), (got, ref) in stacked.items():
        if what == "post":
            errs[f"post/{star}/last_fc.bias"], _ = parity.compare_post(
                {"p": np.array(ref), "g": np.array(stacked[("grad", star)][1])}, "p", "g",
                np.array(got), lr)
        else:
            errs[f"{what}/{star}/last_fc.bias"] = parity.rel_err(got, ref)
    for k, tf in enumerate(tr.tfs):
        for pn, t in tf.state_dict().items():
            errs[f"post/tf{k}/{pn}"] = parity.rel_err(t.cpu().numpy(), orc.Ts[k][pn].numpy())
    return errs


# ------------------------------------------------------------ sweep cases
def sweep_meta(Do, Da, H, P, K, seed=3, **kw):
    """A case of the shape sweep (no reference run): its parameters come from
    ``seed``; the policies' initial actions from a stream of their own."""
    m = dict(kind="ptrain", obs_dim=Do, act_dim=Da, hidden=[H], K=K, P=P, seed=seed, q_min=0.0,
             q_max=50.0, pi_init_w=0.2, q_init_w=0.1, discount=0.99, delta=0.95, lr=3e-4,
             std_lr=1e-4, tau=5e-3, counts=True, n_replay=400)
    m["initial_actions"] = np.random.RandomState(seed + 5).uniform(-0.9, 0.9, P).tolist()
    # particle_trainer.py:61-69
    quant = [i * 1. / (K - 1) for i in range(K)]
    m["delta_index"] = next(i if quant[i] == m["delta"] else i - 1 for i in range(K)
                            if quant[i] >= m["delta"])
    m.update(kw)
    return m


# name -> (meta, B).  The seeds are committed: when a case fails a margin (the
# CPU test measures them on the oracle's own trajectory) its seed changes; no
# row is ever left out.
SWEEP = {
    "smallest": (sweep_meta(2, 1, 4, 1, 2, seed=3), 1),
    "largest": (sweep_meta(2, 1, 4, 16, 16, seed=4), 32),
    "generic_rows": (sweep_meta(3, 2, 68, 5, 5, seed=3), 37),      # stacked widths 340
    "wide_action": (sweep_meta(7, 6, 52, 3, 4, seed=3), 33),
    "batch600": (sweep_meta(5, 2, 24, 3, 3, seed=3), 600),         # split-K slabs, small kernels
    "batch1100": (sweep_meta(5, 2, 24, 3, 3, seed=3), 1100),       # the large-batch kernel set
    "soft": (sweep_meta(5, 3, 24, 3, 3, seed=3, counts=False, soft=0.3), 37),
    "rescale": (sweep_meta(5, 3, 24, 3, 3, seed=3, counts=False, rescale=True, q_max=0.5,
                           q_init_w=0.5), 37),
}
WARMUP = 2   # steps before the compared one: Adam step > 0, moments nonzero


def sweep_batch(meta, B, seed):
    data = synthetic_transitions(max(4 * B, 64), meta["obs_dim"], meta["act_dim"], seed=seed)
    idx = np.random.RandomState(seed).randint(0, len(data["rewards"]), B)
    b = {k: v[idx] for k, v in data.items()}
    if meta["counts"]:
        b["counts"] = np.random.RandomState(seed + 1).randint(0, 2, (B, 1)).astype(np.float64)
    return b


def sweep_margins(meta, B, dtype=torch.float32):
    """(min rank gap, min selection gap) of the compared step (the one after
    WARMUP steps) on the oracle's own trajectory."""
    orc = make_oracle(meta, dtype)
    for s in range(WARMUP + 1):
        out = orc.step(sweep_batch(meta, B, 6 + s))
    return out["min_gap"], out["sel_gap"]
