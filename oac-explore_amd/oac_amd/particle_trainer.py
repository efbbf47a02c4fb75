"""Drop-in ``ParticleTrainer`` of /root/reference/trainer/particle_trainer.py
(12-525): the trainer main.py builds for ``--alg p-oac`` without
``--beta_UB`` (main.py:198-204, 364, 488-490) -- i.e. every reproduce_p-oac*.sh
recipe, at two hidden layers (the Humanoid recipes) or one (main.py's
``--num_layers 1`` default: the riverswim recipes; width a multiple of 4) --
with the shared-layer K-particle critic (``--share_layers``), the
deterministic policy (``deterministic = not --stochastic``), and optionally
``--counts`` / ``std_soft_update`` / ``--mean_update`` /
``rescale_targets_around_mean``.  Per step: sorted-particle TD targets with
the critic loss averaged over particles, the policy maximising the
``delta_index``-th sorted particle of the post-step critic, the target policy
its particle mean, Polyak.  The step runs in liboac_amd (csrc/det_plan.hip);
the interface is the reference's: constructor kwargs, ``train`` /
``train_from_torch``, ``predict``, ``obj_func``, ``get_diagnostics``,
``end_epoch``, ``networks``, ``get_snapshot`` / ``restore_from_snapshot``,
``qfs`` / ``tfs`` / ``qf_optimizers`` / ``target_policy``.

``ensemble=True, n_policies=P`` (main.py's ``--ensemble``; with separate critics
at one hidden layer, 1 <= P <= 16: w_oac_mountain_no_resampling.sh): P
separately optimised policies, stored stacked; the TD target's next action is
the best of the P proposals under the online critics' upper bound, policy p
ascends its own upper bound, and ``policy`` is an ``ArenaEnsemblePolicy`` that
acts the same way (particle_trainer.py:115-137, 203-206, 321-338;
``policy_optimizers``, the reference's ``networks``, statistics and snapshot
keys).
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .tp_trainer import _TargetPolicyTrainer


class ParticleTrainer(_TargetPolicyTrainer):
    _kind = _lib.OAC_KIND_PARTICLE_UB

    def __init__(self, policy_producer, q_producer, n_estimators=2, action_space=None,
                 discount=0.99, reward_scale=1.0, delta=0.95, policy_lr=1e-3, qf_lr=1e-3,
                 optimizer_class=None, soft_target_tau=1e-2, target_update_period=1,
                 use_automatic_entropy_tuning=False, target_entropy=None, deterministic=True,
                 q_min=0, q_max=100, ensemble=False, n_policies=1, share_layers=False,
                 r_mellow_max=1., b_mellow_max=None, mellow_max=False, counts=False,
                 mean_update=False, global_opt=False, std_soft_update=False,
                 std_soft_update_prob=0., train_bias=True, use_target_policy=False,
                 rescale_targets_around_mean=False,
                 device=None, seed=0, use_graph=False, gemm_cfg=-1):
        unsupported = dict(deterministic=not deterministic)
        if ensemble:
            # the policy ensemble (particle_trainer.py:115-137) runs with separate
            # critics at one hidden layer, as direct launches on one process; the
            # options it does not take, every one by name
            unsupported.update(
                share_layers=share_layers, global_opt=global_opt, use_graph=use_graph,
                mellow_max=mellow_max,
                # (the reference's constructor fails here: soft_update_from_to of an EnsemblePolicy)
                use_target_policy=use_target_policy and not mean_update,
                n_policies=not (isinstance(n_policies, (int, np.integer)) and 1 <= n_policies <= 16))
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(
                "oac_amd.ParticleTrainer implements the p-oac recipe configurations "
                "(share_layers=True, or one critic per particle at one hidden layer; "
                "deterministic policy, counts / std_soft_update / "
                "mean_update / rescale_targets_around_mean / train_bias / "
                "use_target_policy, global_opt; ensemble=True with 1 <= n_policies <= 16 for "
                "share_layers=False at one hidden layer, without global_opt / use_graph / "
                "mellow_max, and use_target_policy only with mean_update); "
                f"unsupported: {bad if not ensemble else ['ensemble'] + bad}")
        assert not counts or not std_soft_update   # particle_trainer.py:92
        self._common_init(device, soft_target_tau, target_update_period, deterministic,
                          discount, reward_scale, policy_lr, qf_lr, use_graph, seed, gemm_cfg)
        self.train_bias = train_bias
        self.unshared = not share_layers
        if self.unshared and not 2 <= n_estimators <= 16:
            raise NotImplementedError(
                f"oac_amd.ParticleTrainer with share_layers=False takes 2 to 16 particles, got "
                f"n_estimators={n_estimators}; unsupported: ['n_estimators']")
        # quantile bookkeeping, particle_trainer.py:61-69 (delta_index uses p - 1
        # when the quantile grid steps over delta)
        quantiles = [i * 1. / (n_estimators - 1) for i in range(n_estimators)]
        for p in range(n_estimators):
            if quantiles[p] == delta:
                self.delta_index = p
                break
            if quantiles[p] > delta:
                self.delta_index = p - 1
                break
        self.share_layers = share_layers
        self.num_particles = n_estimators
        self.n_estimators = n_estimators if self.unshared else 1   # particle_trainer.py:72-77
        self._q_out = n_estimators
        self.q_min, self.q_max, self.delta = q_min, q_max, delta
        self.r_mellow_max, self.b, self.mellow_max = r_mellow_max, b_mellow_max, mellow_max
        self.counts, self.mean_update, self.global_opt = counts, mean_update, global_opt
        self.std_soft_update, self.std_soft_update_prob = std_soft_update, std_soft_update_prob
        self.rescale_targets_around_mean = rescale_targets_around_mean
        self.action_space = action_space
        self.ensemble, self.n_policies = ensemble, n_policies
        self.use_target_policy = use_target_policy

        # producer call order of the reference constructor: SACTrainer's policy
        # and four critics (unused), the shared-layer critic and its target
        # (the target then copied from the critic, soft_update tau=1), then
        # target_policy (particle_trainer.py:47-59, 96-106, 141)
        if self.unshared:
            self._reject_unshared_options()
        ref_pol = policy_producer()
        for _ in range(4):
            q_producer()
        init_values = np.linspace(q_min, q_max, n_estimators)
        if self.unshared:
            # particle_trainer.py:105-114: per particle a critic and its target
            # (the target then copied from the critic), biased at its initial value
            ref_q = []
            for i in range(n_estimators):
                ref_q.append(q_producer(bias=init_values[i], train_bias=train_bias))
                q_producer(bias=init_values[i], train_bias=train_bias)
        else:
            ref_q = q_producer(bias=init_values, train_bias=train_bias)
            q_producer(bias=init_values, train_bias=train_bias)
        if ensemble:
            # particle_trainer.py:117-127: each policy starts biased at an initial
            # action.  Da > 1 draws P Da values on numpy's global stream and
            # EnsemblePolicy uses the first P of them, one per policy, filled into
            # every action dimension (policies.py:569, 224-225) -- kept as it is.
            if action_space.shape[0] > 1:
                initial_actions = np.random.uniform(
                    low=action_space.low, high=action_space.high,
                    size=(n_policies, action_space.shape[0])).flatten()
            else:
                initial_actions = np.linspace(-1., 1., n_policies)
                initial_actions[0] += 5e-2
                initial_actions[-1] -= 5e-2
            self.initial_actions = initial_actions
            ref_pol = policy_producer(bias=initial_actions, ensemble=ensemble,
                                      n_policies=n_policies, approximator=self,
                                      share_layers=share_layers)
        ref_init = policy_producer() if global_opt else None
        ref_tp = policy_producer()
        ref_init_tp = policy_producer() if global_opt else None
        if self.unshared:
            K = n_estimators
            self._build(ref_pol, ref_q, ref_q, ref_tp, policy_lr, [qf_lr] * K,
                        positives=[False] * K, frozen=[not train_bias] * K)
        else:
            self._build(ref_pol, ref_q, ref_q, ref_tp, policy_lr, qf_lr)
        self._make_init_policies(ref_init, ref_init_tp)
        self._make_target_policy_network(policy_producer)

    def _make_cfg(self, batch):
        c = super()._make_cfg(batch)
        c.delta_index = int(self.delta_index)
        c.rescale_spread = float(self.q_max - self.q_min) if self.rescale_targets_around_mean \
            else 0.0
        return c

    # ------------------------------------------------------------ diagnostics
    def _fill_eval_statistics(self, plan):
        """particle_trainer.py:362-403 (keys and order; 'Policy Loss' is
        mean(upper bound) and 'Policy mu' / 'Policy log std' describe the
        target policy, as in the reference)."""
        v = {k: t.detach().to("cpu").numpy() for k, t in plan.views.items()
             if k in ("q1", "tq1", "sqe1", "qnew", "head3")}
        K, Da = self.num_particles, self.act_dim
        qs, tq = v["q1"], v["tq1"]
        sorted_qs = np.sort(qs, axis=1).T[:, :, None]          # [K, B, 1]
        order = np.arange(K)[None, :]
        losses = [np.float32(np.mean(v["sqe1"][:, i])) for i in range(K)]
        st = OrderedDict()
        st["QF mean"] = np.mean(sorted_qs, axis=0).mean()
        st["QF std"] = np.std(sorted_qs, axis=0).mean()
        st["QF Unordered"] = np.float64(np.sum(np.argsort(qs, axis=1, kind="stable") != order))
        st["QF target Undordered"] = np.float64(
            np.sum(np.argsort(tq, axis=1, kind="stable") != order))
        # (:267 divides the summed loss by the particle count with share_layers only)
        st["Q Loss"] = np.float32(np.sum(losses, dtype=np.float32)) if self.unshared else \
            np.float32(np.sum(losses, dtype=np.float32) / np.float32(K))
        for i in range(K):
            st[f"QF{i} Loss"] = losses[i]
            self._stats(st, f"Q{i}Predictions", sorted_qs[i])
            self._stats(st, f"Q{i}Targets", tq[:, i:i + 1])
        if not self.global_opt:   # (:422 / :418: the step has no policy loss)
            st["Policy Loss"] = np.mean(v["qnew"])
        self._stats(st, "Policy mu", v["head3"][:, :Da])
        self._stats(st, "Policy log std", np.clip(v["head3"][:, Da:], -20, 2))
        self.eval_statistics = st

    # ------------------------------------------------------------ misc API
    def _sorted(self, obs, action):
        with torch.no_grad():
            obs, action = self._tensor(obs), self._tensor(action)
            if self.unshared:   # particle_trainer.py:163-166: one call per critic, stacked
                qs = torch.stack([q(obs, action) for q in self.qfs], dim=0)
            else:
                qs = self.qfs[0](obs, action).t().unsqueeze(-1)
        return qs, torch.sort(qs, dim=0)[0]                     # [K, B, 1]

    def predict(self, obs, action, all_particles=False):
        """particle_trainer.py:160-174."""
        _, sorted_qs = self._sorted(obs, action)
        upper_bound = sorted_qs[self.delta_index]
        if all_particles:
            return sorted_qs, upper_bound
        return upper_bound

    def obj_func(self, states, actions, upper_bound=False):
        """particle_trainer.py:507-518."""
        qs, sorted_qs = self._sorted(states, actions)
        return sorted_qs[self.delta_index] if upper_bound else torch.mean(qs, dim=0)
