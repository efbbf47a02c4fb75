"""Drop-in ``DDPGTrainer`` (/root/reference/trainer/ddpg_trainer.py:13-237, the
trainer of ``--alg ddpg``, main.py:184-190) running the gradient step in
liboac_amd on the GPU (csrc/ddpg_plan.hip, OAC_KIND_DDPG).

One critic and its target, the deterministic policy (the reference forces
``deterministic=True``, :37) and, with ``use_target_policy``, the
``target_policy_network`` that supplies the next actions of the TD target.
The reference soft-updates that network onto itself (:152-155), so it stays
the copy of the initial policy made at construction (:66-70): here a frozen
block outside the Adam arena (oac_sac_buffers.next_policy), loadable like the
reference's.

The step keeps the reference's torch-1.4 update order: the
critic steps before ``policy_loss.backward()`` (:136-142), so the policy
gradient flows through the post-step critic weights with the pre-step
activations and ReLU masks.

Interface kept from the reference: constructor kwargs, ``train`` /
``train_from_torch``, ``predict``, ``get_diagnostics``, ``end_epoch``,
``networks``, ``get_snapshot`` / ``restore_from_snapshot``, ``policy``, ``qf``,
``target_qf``, ``qfs``, ``tfs``, ``policy_optimizer``, ``qf_optimizer``.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .networks import ArenaFlattenMlp, ArenaTanhGaussianPolicy, _as_input, critics_apply
from .trainer import AdamStateView, _ArenaTrainer, _dims_from_state, _plain_stats, _twin_views

_LOG_STD_HEAD = ("last_fc_log_std.weight", "last_fc_log_std.bias")


def _fixed_std_of(ref_pol, pol_sd):
    """The producer-built policy's fixed std as a float64 array, or None for
    the learned-std policy: ``std is not None`` (policies.py:236-249), or a
    state_dict without ``last_fc_log_std.*``."""
    std = getattr(ref_pol, "std", None)
    has_head = any(k in pol_sd for k in _LOG_STD_HEAD)
    if std is None:
        if has_head:
            return None
        raise ValueError("the policy has no last_fc_log_std parameters and no std attribute")
    if torch.is_tensor(std):
        std = std.detach().cpu().numpy()
    return np.asarray(std, np.float64)


class DDPGTrainer(_ArenaTrainer):
    """DDPGTrainer (trainer/ddpg_trainer.py:13) on liboac_amd."""

    _kind = _lib.OAC_KIND_DDPG
    _q_out = 1

    def __init__(self, policy_producer, q_producer, action_space=None, discount=0.99,
                 reward_scale=1.0, policy_lr=1e-3, qf_lr=1e-3, optimizer_class=None,
                 soft_target_tau=1e-2, target_update_period=1, deterministic=True,
                 use_target_policy=False, device=None, seed=0, gemm_cfg=-1):
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        self.use_automatic_entropy_tuning = False   # (no entropy term in this step)
        self.target_entropy = 0.0
        self.soft_target_tau = soft_target_tau
        self.target_update_period = target_update_period
        self.deterministic = True                    # ddpg_trainer.py:37
        self.discount, self.reward_scale = discount, reward_scale
        self.use_target_policy = use_target_policy
        self.policy_lr, self.qf_lr = policy_lr, qf_lr
        self.action_space = action_space
        self.use_graph = False   # OAC_KIND_DDPG issues its launches directly
        self.seed, self._gemm_cfg = int(seed), gemm_cfg

        # producer call order of the reference constructor (:47-49, :66-67)
        ref_pol, ref_q, ref_qt = policy_producer(), q_producer(), q_producer()
        pol_sd = {k: v.detach() for k, v in ref_pol.state_dict().items()}
        std = _fixed_std_of(ref_pol, pol_sd)
        Do, Da, H, Q = _dims_from_state(pol_sd, ref_q.state_dict(), fixed_std=std is not None)
        if Q != 1:
            raise ValueError("DDPGTrainer's critic has one output")
        lay = self._alloc(Do, Da, H, self.device)
        self.policy = ArenaTanhGaussianPolicy(self.params, 0, lay, Do, Da, H, std=std)
        self.qf = ArenaFlattenMlp(self.params, lay.q1_base, lay, Do, Da, H, 1)
        self.target_qf = ArenaFlattenMlp(self.targets, 0, lay, Do, Da, H, 1)
        self.policy.load_state_dict(pol_sd)
        self.qf.load_state_dict({k: v.detach() for k, v in ref_q.state_dict().items()})
        self.target_qf.load_state_dict({k: v.detach() for k, v in ref_qt.state_dict().items()})
        self.policy.oac_trainer = self
        self.qfs, self.tfs = [self.qf], [self.target_qf]
        tw = lambda other, mod: _twin_views(self.params, other, list(mod.parameters()))
        # the deterministic policy's log-std head (if it has one) never gets a gradient
        no_grad = [i for i, (n, _) in enumerate(self.policy.named_parameters())
                   if n in _LOG_STD_HEAD]
        self.policy_optimizer = AdamStateView(self, list(self.policy.parameters()),
                                              tw(self.adam_m, self.policy),
                                              tw(self.adam_v, self.policy), policy_lr,
                                              (0.9, 0.999), 1e-8, no_grad=no_grad)
        self.qf_optimizer = AdamStateView(self, list(self.qf.parameters()),
                                          tw(self.adam_m, self.qf), tw(self.adam_v, self.qf),
                                          qf_lr, (0.9, 0.999), 1e-8)
        self.eval_statistics = OrderedDict()
        self._n_train_steps_total = 0
        self._need_to_update_eval_statistics = True
        self.target_policy_network = None
        self._tpn = None
        if use_target_policy:
            policy_producer()   # the reference's producer call (its init is overwritten, :68-70)
            self._tpn = self.params[:lay.pol_size].clone()
            self.target_policy_network = ArenaTanhGaussianPolicy(self._tpn, 0, lay, Do, Da, H,
                                                                 std=std)

    def _next_policy_ptr(self):
        return None if self._tpn is None else self._tpn.data_ptr()

    # ------------------------------------------------------------ diagnostics
    def _fill_eval_statistics(self, plan):
        """ddpg_trainer.py:160-183 (keys and order)."""
        v = {k: t.detach().to("cpu").numpy() for k, t in plan.views.items()
             if k in ("q1", "y", "sqe1", "qnew", "head1")}
        st = OrderedDict()
        st["QF mean"] = np.mean(v["q1"], axis=0).mean()
        st["Q Loss"] = np.float32(np.mean(v["sqe1"]))
        st["Policy Loss"] = np.mean(-v["qnew"])
        for name, arr in (("Q Predictions", v["q1"]), ("Q Targets", v["y"]),
                          ("Policy mu", v["head1"][:, :self.act_dim])):
            st[name + " Mean"] = np.mean(arr)
            st[name + " Std"] = np.std(arr)
            st[name + " Max"] = np.max(arr)
            st[name + " Min"] = np.min(arr)
        self.eval_statistics = st

    def get_diagnostics(self):
        return self.eval_statistics

    def end_epoch(self, epoch):
        self._need_to_update_eval_statistics = True

    # ------------------------------------------------------------ misc API
    def predict(self, obs, action):
        """ddpg_trainer.py:78-88.  The reference indexes a module there
        (``self.qf[0]``, :87), which cannot run; the evident intent is
        implemented: Q(obs, action) of the critic, a 1-D observation / action
        pair evaluated as a batch of one."""
        obs, action = _as_input(obs, self.device), _as_input(action, self.device)
        if obs.dim() == 1:
            obs, action = obs.unsqueeze(0), action.unsqueeze(0)
        return critics_apply([self.qf], obs, action)

    @property
    def networks(self):
        nets = [self.policy, self.qf, self.target_qf]
        if self.use_target_policy:
            nets.append(self.target_policy_network)
        return nets

    def get_snapshot(self):
        """ddpg_trainer.py:203-217 (keys).  ``target_policy_network`` is stored
        as its state dict (the reference stores the module), so the snapshot
        loads with ``torch.load(weights_only=True)``."""
        snapshot = dict(
            policy_state_dict=self.policy.state_dict(),
            policy_optim_state_dict=self.policy_optimizer.state_dict(),
            qf_state_dict=self.qf.state_dict(),
            qf_optim_state_dict=self.qf_optimizer.state_dict(),
            target_qf_state_dict=self.target_qf.state_dict(),
            eval_statistics=_plain_stats(self.eval_statistics),
            _n_train_steps_total=self._n_train_steps_total,
            _need_to_update_eval_statistics=self._need_to_update_eval_statistics,
        )
        if self.use_target_policy:
            snapshot["target_policy_network"] = self.target_policy_network.state_dict()
        return snapshot

    def restore_from_snapshot(self, ss):
        """ddpg_trainer.py:219-237.  The reference tuple-unpacks a state dict
        (:225) and writes ``_need_to_update_eval_statistic`` without the final
        s (:237), so it cannot run as written; the evident intent is
        implemented: every key of ``get_snapshot`` is restored.
        ``target_policy_network`` may be a state dict or a module."""
        self.policy.load_state_dict(ss["policy_state_dict"])
        self.policy_optimizer.load_state_dict(ss["policy_optim_state_dict"])
        self.qf.load_state_dict(ss["qf_state_dict"])
        self.qf_optimizer.load_state_dict(ss["qf_optim_state_dict"])
        self.target_qf.load_state_dict(ss["target_qf_state_dict"])
        if self.use_target_policy:
            tpn = ss["target_policy_network"]
            if hasattr(tpn, "state_dict"):
                tpn = tpn.state_dict()
            self.target_policy_network.load_state_dict(tpn)
        self.eval_statistics = ss["eval_statistics"]
        self._n_train_steps_total = int(ss["_n_train_steps_total"])
        self._need_to_update_eval_statistics = ss["_need_to_update_eval_statistics"]
        self.step_state[0] = self._n_train_steps_total
