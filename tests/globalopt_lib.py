"""Shared pieces of the ``global_opt`` tests of the g-oac GaussianTrainer and
the p-oac ParticleTrainer: the CPU restatement of the option -- the train step
that leaves the policy alone (gaussian_trainer.py:337-341,
particle_trainer.py:343-346) and the sweep of utils/core.py:64-137
``optimize_policy`` -- built from oracle.sac_oracle's functions, its errors
against a fixture, and the oac_amd trainer for a fixture.  Used by
tests/golden/make_golden_globalopt.py (the seed condition), the CPU test and
the GPU tests."""
import math
import random

import numpy as np
import torch

import parity
import shallow_lib as sl
import test_oracle_golden as tog
from fixtures_lib import synthetic_transitions
from gpu_helpers import Space, StateDictModule
from oracle import sac_oracle as so

FIXTURES = ["goac_go_d1", "ptrain_go_d1_mean_counts", "ptrain_go_d2"]
# the fixtures' sequence: train steps and optimize_policy calls (iterations)
SEQUENCE = (("train", 2), ("sweep", 4), ("train", 1), ("sweep", 3))
LOG_STD = ("last_fc_log_std.weight", "last_fc_log_std.bias")


def reference_shuffle_indices(n, iterations):
    """Row indices of every iteration's batch: the reference's cumulative
    ``random.shuffle(dataset)`` (core.py:74) replayed on an index column, from
    the global ``random`` stream's current state."""
    col = np.arange(n).reshape(n, 1)
    out = []
    for _ in range(iterations):
        random.shuffle(col)
        out.append(col[:, 0].copy())
    return out


def init_params(meta):
    """init_policy / init_target_policy weights of a fixture (own seeds)."""
    return (sl.params_of(dict(meta, seed=meta["seed"] + 200))["policy"],
            sl.params_of(dict(meta, seed=meta["seed"] + 201))["policy"])


def dataset_of(meta):
    """get_dataset() of the fixture's replay: its observations."""
    tr = synthetic_transitions(meta["n_replay"], meta["obs_dim"], meta["act_dim"], seed=0)
    return np.asarray(tr["observations"])


class Restatement:
    """The oracle of the fixture's trainer with global_opt=True."""

    def __init__(self, meta, dtype=torch.float32, g=None, params=None):
        self.meta, self.dtype = meta, dtype
        self.orc = sl.make_oracle(meta, dtype, g, params=params)
        self.init = so.to_torch_params(init_params(meta)[0], dtype)

    def train(self, batch):
        """One train step: the oracle's, with the policy's part taken back --
        the policy's update touches neither the critic nor the target policy
        (det_plan.hip's header), so the rest of the step is what the
        reference's global_opt branch computes."""
        o = self.orc
        keep = [{k: v.clone() for k, v in d.items()} for d in (o.P, o.opt_p.m, o.opt_p.v)]
        t = o.opt_p.t
        out = o.step(batch)
        for d, src in zip((o.P, o.opt_p.m, o.opt_p.v), keep):
            for k, v in src.items():
                d[k].copy_(v)
        o.opt_p.t = t
        return out

    def upper_bound_seed(self, q, N):
        """(ub [N, 1], dL/dq [N, K]) of L = -mean(obj_func(upper_bound=True))."""
        o = self.orc
        g0 = -torch.ones(N, 1, dtype=self.dtype) / N
        if self.meta["kind"] == "goac":            # gaussian_trainer.py:519-529
            qs, stds = q[:, :1], torch.exp(q[:, 1:2])
            return qs + o.z * stds, torch.cat([g0, g0 * o.z * stds], dim=1)
        pq = q.t()                                  # particle_trainer.py:507-518
        sq, sidx = torch.sort(pq, dim=0)
        d = o.delta_index
        seed = torch.zeros_like(pq).scatter_(0, sidx[d:d + 1], g0.t()).t()
        return sq[d][:, None], seed

    def iteration(self, obs):
        """One sweep iteration on the rows ``obs`` (core.py:80-99): the policy
        gradient, the loss, grad_norm(policy); then the policy's Adam step."""
        o = self.orc
        obs = so._t(obs, self.dtype)
        N = obs.shape[0]
        pf = so.policy_forward(obs, o.P, None, deterministic=True)
        cn = so.q_forward(obs, pf["a"], o.Q)
        ub, seed = self.upper_bound_seed(cn["q"], N)
        da = so.q_input_grad(cn, seed, o.Q)[:, o.Do:]
        g = so.det_policy_backward(pf, o.P, da)
        loss = float(-ub.mean())
        gn = math.sqrt(sum(float(v.norm(2)) ** 2 for k, v in g.items() if k not in LOG_STD))
        o.opt_p.step(g)
        return g, loss, gn

    def sweep(self, data, rows_per_iteration):
        """optimize_policy: restart from init_policy, one iteration per entry
        of ``rows_per_iteration`` (index arrays into ``data``)."""
        for k, v in self.init.items():
            self.orc.P[k].copy_(v)
        return [self.iteration(data[idx]) for idx in rows_per_iteration]


def restatement_errors(meta, g, dtype=torch.float32):
    """{key: error} of the restatement's run of the fixture's sequence against
    everything the reference recorded."""
    rs = Restatement(meta, dtype, g)
    orc = rs.orc
    pol_order, q_order = sl.orders(len(meta["hidden"]))
    data = dataset_of(meta)
    errs = {}
    s = c = 0
    for what, n in SEQUENCE:
        if what == "train":
            for _ in range(n):
                b = tog.build_batch(meta, g[f"s{s}/idx"])
                if meta["counts"]:
                    b["counts"] = g[f"s{s}/counts"][:, None]
                out = rs.train(b)
                for grp in ("target_policy", "qf"):
                    for pn in (q_order if grp == "qf" else pol_order):
                        key = f"s{s}/grad/{grp}/{pn}"
                        errs[key] = parity.compare(g, key, out["grads"][grp][pn].numpy())
                for grp, params_ in (("policy", orc.P), ("target_policy", orc.TP),
                                     ("qf", orc.Q), ("tf", orc.T)):
                    for pn, t in params_.items():
                        key = f"s{s}/post/{grp}/{pn}"
                        gk = f"s{s}/grad/{grp}/{pn}" if s == 0 and grp in ("target_policy", "qf") \
                            else None
                        errs[key], _ = parity.compare_post(g, key, gk, t.numpy(), meta["lr"])
                errs.update(tog.stat_errors(s, g, sl.stats_of(meta, out)))
                s += 1
            continue
        its = rs.sweep(data, [g[f"c{c}/i{k}/rows"] for k in range(n)])
        for k, (grads, loss, gn) in enumerate(its):
            for pn in pol_order:
                key = f"c{c}/i{k}/grad/policy/{pn}"
                errs[key] = parity.compare(g, key, grads[pn].numpy())
            errs[f"c{c}/i{k}/loss"] = parity.rel_err(np.array([loss]), g[f"c{c}/i{k}/loss"])
            errs[f"c{c}/i{k}/grad_norm"] = parity.rel_err(np.array([gn]),
                                                          g[f"c{c}/i{k}/grad_norm"])
        for pn in pol_order:
            errs[f"c{c}/post/policy/{pn}"] = parity.compare(g, f"c{c}/post/policy/{pn}",
                                                            orc.P[pn].numpy())
            if pn in LOG_STD:
                continue
            errs[f"c{c}/opt/exp_avg/{pn}"] = parity.compare(g, f"c{c}/opt/exp_avg/{pn}",
                                                            orc.opt_p.m[pn].numpy())
            errs[f"c{c}/opt/exp_avg_sq/{pn}"] = parity.compare(g, f"c{c}/opt/exp_avg_sq/{pn}",
                                                               orc.opt_p.v[pn].numpy())
        assert orc.opt_p.t == int(g[f"c{c}/opt/step"])
        c += 1
    return errs


def producers(meta, params=None):
    """Producers in the reference constructors' call order with global_opt:
    policy, init_policy, target_policy, init_target_policy (then the
    use_target_policy network); four unused critics, the critic, its target."""
    params = sl.params_of(meta) if params is None else params
    ip, itp = init_params(meta)
    pols = iter([params["policy"], ip, params["target_policy"], itp, params["policy"]])
    qs = iter([params["qf1"]] * 4 + [params["qf1"], params["target_qf1"]])
    return (lambda **k: StateDictModule(next(pols)),
            lambda **k: StateDictModule(next(qs)))


def trainer_for(meta, params=None, global_opt=True, **kw):
    """The oac_amd trainer of a fixture's meta, built with global_opt."""
    import oac_amd
    pp, qp = producers(meta, params) if global_opt else sl.det_producers(
        sl.params_of(meta) if params is None else params)
    common = dict(action_space=Space(meta["act_dim"]), discount=meta["discount"],
                  reward_scale=1.0, delta=meta["delta"], policy_lr=meta["lr"],
                  qf_lr=meta["lr"], soft_target_tau=meta["tau"], target_update_period=1,
                  q_min=meta["q_min"], q_max=meta["q_max"], share_layers=True,
                  counts=bool(meta.get("counts")), mean_update=bool(meta.get("mean_update")),
                  train_bias=meta.get("train_bias", True), global_opt=global_opt)
    common.update(kw)
    if meta["kind"] == "goac":
        return oac_amd.GaussianTrainer(pp, qp, n_estimators=2, **common)
    return oac_amd.ParticleTrainer(pp, qp, n_estimators=meta["K"], **common)


class NumpyDataset:
    """A buffer that only has the reference's get_dataset()."""

    def __init__(self, data):
        self.data = np.asarray(data)

    def get_dataset(self):
        return self.data
