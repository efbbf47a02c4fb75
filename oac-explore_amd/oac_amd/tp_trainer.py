"""Shared host side of the deterministic-policy trainers with a separately
trained ``target_policy`` -- g-oac ``GaussianTrainer``
(/root/reference/trainer/gaussian_trainer.py) and the p-oac
``ParticleTrainer`` (/root/reference/trainer/particle_trainer.py).  Both are
``SACTrainer`` subclasses in the reference with the same network set
(policy, one shared-layer critic and its target, target_policy), the same
optimizer set and the same snapshot keys; their steps run in liboac_amd
(csrc/det_plan.hip) over the arena [policy | target_policy | critic].

With ``share_layers=False`` (the reference's default; one hidden layer) the
critic block holds the K separate one-output critics stacked -- q and std
(g-oac) or one per particle (p-oac) -- and ``qfs`` / ``tfs`` /
``qf_optimizers`` are K modules / optimizer views over their slices.
"""
import ctypes
import random
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_ptr
from .networks import ArenaEnsemblePolicy, ArenaFlattenMlp, ArenaTanhGaussianPolicy
from .trainer import AdamStateView, _ArenaTrainer, _dims_from_state, _twin_views, _plain_stats

_LOG_STD_HEAD = ("last_fc_log_std.weight", "last_fc_log_std.bias")


def shuffle_gather_indices(n):
    """``J`` with ``new[i] = old[J[i]]`` for one ``random.shuffle`` of an n-row
    2-D numpy array as utils/core.py:74 performs it -- drawn from the global
    ``random`` stream exactly as ``shuffle`` draws (``_randbelow(i + 1)`` for
    i = n-1 .. 1).  Python's swap ``x[i], x[j] = x[j], x[i]`` evaluates two row
    VIEWS on the right, so row j is copied over row i and row i's value is
    lost: the shuffle duplicates rows instead of permuting them.  j <= i and
    position j is overwritten only later, so each shuffle is a gather."""
    below = getattr(random.shuffle.__self__, "_randbelow", None) or random.randrange
    J = np.zeros(n, np.int64)
    J[:0:-1] = [below(i + 1) for i in range(n - 1, 0, -1)]
    return J


class _TargetPolicyTrainer(_ArenaTrainer):
    _positive = False       # critic output exp (FlattenMlp positive=..., networks.py:69-75)

    def _common_init(self, device, soft_target_tau, target_update_period, deterministic,
                     discount, reward_scale, policy_lr, qf_lr, use_graph, seed, gemm_cfg):
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        # SACTrainer.__init__ bookkeeping (no entropy term in these steps)
        self.use_automatic_entropy_tuning = False
        self.target_entropy = 0.0
        self.soft_target_tau, self.target_update_period = soft_target_tau, target_update_period
        self.deterministic, self.discount, self.reward_scale = deterministic, discount, reward_scale
        self.policy_lr, self.qf_lr = policy_lr, qf_lr
        self.use_graph, self.seed, self._gemm_cfg = use_graph, int(seed), gemm_cfg

    unshared = False        # share_layers=False: separate one-output critics (oac_sac_config.unshared)
    ensemble = False        # ParticleTrainer(ensemble=True): n_policies stacked policies
    n_policies = 1
    std_lr = 0.0

    def _reject_unshared_options(self):
        """share_layers=False runs as direct launches on one process, without
        the policy sweep: the options it does not take, by name."""
        bad = [k for k, v in dict(global_opt=self.global_opt, use_graph=self.use_graph).items() if v]
        if bad:
            raise NotImplementedError(
                f"oac_amd.{type(self).__name__} with share_layers=False (separate critics, each "
                f"with its own optimizer) does not implement {' / '.join(bad)}; unsupported: {bad}")

    def _build(self, ref_pol, ref_q, ref_qt, ref_tp, policy_lr, qf_lr, positives=None, frozen=None):
        """Arena modules initialised from the producers' state_dicts, and the
        reference's optimizer views (policy, target_policy, shared critic).
        share_layers=False (``self.unshared``): ``ref_q`` / ``ref_qt`` /
        ``qf_lr`` / ``positives`` / ``frozen`` are lists over the K one-output
        critics, stored stacked in one critic block (include/oac_amd.h), each
        exposed through modules and an optimizer view of its own slices."""
        ens = list(ref_pol.policies) if self.ensemble else None   # EnsemblePolicy, or any .policies
        if ens is not None and len(ens) != self.n_policies:
            raise ValueError(f"ensemble: policy_producer built {len(ens)} policies, "
                             f"n_policies={self.n_policies}")
        pol_sd = {k: v.detach() for k, v in (ens[0] if ens else ref_pol).state_dict().items()}
        q0 = ref_q[0] if self.unshared else ref_q
        Do, Da, H, K, self.n_hidden = _dims_from_state(pol_sd, q0.state_dict(), depths=(1, 2))
        if ens is not None and self.n_hidden != 1:
            raise NotImplementedError(
                f"oac_amd.{type(self).__name__}: ensemble=True is implemented for one hidden layer "
                f"(--num_layers 1, the w_oac recipe); got {self.n_hidden} hidden layers; "
                f"unsupported: ['ensemble', 'num_layers']")
        if self.unshared and self.n_hidden != 1:
            raise NotImplementedError(
                f"oac_amd.{type(self).__name__}: share_layers=False is implemented for one hidden "
                f"layer (--num_layers 1, the recipes that run without --share_layers); got "
                f"{self.n_hidden} hidden layers; unsupported: ['share_layers', 'num_layers']")
        if self.n_hidden == 1 and H % 4:
            raise ValueError(f"one hidden layer: the width must be a multiple of 4, got {H}")
        if self.unshared and K != 1:
            raise ValueError(f"share_layers=False: q_producer must build critics with one output "
                             f"(main.py:138-143), got {K}")
        if not self.unshared and K != self._q_out:
            raise ValueError(f"share_layers: q_producer must build a critic with {self._q_out} "
                             f"outputs, got {K}")
        self._ens_policies = self.n_policies if ens is not None else 0
        lay = self._alloc(Do, Da, H, self.device)
        if ens is not None:
            # the P policies stacked in front of the target_policy block
            # (oac_ensemble_layout); `policy` acts as the reference's EnsemblePolicy
            self.policy = ArenaEnsemblePolicy(self.params, self.ens_layout, Do, Da, H, self)
            self.policy.load_state_dict(
                [{k: v.detach() for k, v in m.state_dict().items()} for m in ens])
        else:
            self.policy = ArenaTanhGaussianPolicy(self.params, 0, lay, Do, Da, H)
            self.policy.load_state_dict(pol_sd)
        self.target_policy = ArenaTanhGaussianPolicy(self.params, lay.tpol_base, lay, Do, Da, H)
        self.target_policy.load_state_dict({k: v.detach() for k, v in ref_tp.state_dict().items()})
        self.policy.oac_trainer = self
        if self.unshared:
            assert lay.n_critics == self._q_out == len(ref_q) == len(ref_qt)
            self.qfs, self.tfs = [], []
            for k in range(self._q_out):
                qf = ArenaFlattenMlp(self.params, lay.q1_base, lay, Do, Da, H, 1,
                                     positive=positives[k], stacked_index=k)
                tf = ArenaFlattenMlp(self.targets, 0, lay, Do, Da, H, 1,
                                     positive=positives[k], stacked_index=k)
                qf.load_state_dict({n: v.detach() for n, v in ref_q[k].state_dict().items()})
                tf.load_state_dict({n: v.detach() for n, v in ref_qt[k].state_dict().items()})
                self.qfs.append(qf)
                self.tfs.append(tf)
        else:
            qf = ArenaFlattenMlp(self.params, lay.q1_base, lay, Do, Da, H, K, positive=self._positive)
            tf = ArenaFlattenMlp(self.targets, 0, lay, Do, Da, H, K, positive=self._positive)
            qf.load_state_dict({k: v.detach() for k, v in ref_q.state_dict().items()})
            tf.load_state_dict({k: v.detach() for k, v in ref_qt.state_dict().items()})
            self.qfs, self.tfs = [qf], [tf]
        tw = lambda other, mod: _twin_views(self.params, other, list(mod.parameters()))
        names = [n for n, _ in (self.policy.policies[0] if ens else self.policy).named_parameters()]
        # deterministic policies: the log-std heads never get a gradient
        no_grad = [i for i, n in enumerate(names) if n in _LOG_STD_HEAD]

        def popt(mod, step_source=None):
            return AdamStateView(self, list(mod.parameters()), tw(self.adam_m, mod),
                                 tw(self.adam_v, mod), policy_lr, (0.9, 0.999), 1e-8,
                                 no_grad=no_grad, step_source=step_source)
        # global_opt: the policy's optimizer is stepped by optimize_policies
        # alone (utils/core.py:98), so its `step` counts sweep iterations
        self._policy_opt_steps = 0
        if ens is not None:
            # particle_trainer.py:128-137: one Adam per policy, all stepped once per
            # train step; SACTrainer's policy_optimizer stays, over the discarded
            # parent policy, and is never stepped (no state; a snapshot key only)
            self.policy_optimizers = [popt(pol) for pol in self.policy.policies]
            self.policy_optimizer = AdamStateView(
                self, list(self.policy.policies[0].parameters()), [], [], policy_lr, (0.9, 0.999),
                1e-8, step_source=lambda: 0)
        else:
            self.policy_optimizer = popt(
                self.policy, (lambda: self._policy_opt_steps) if self.global_opt else None)
        self.target_policy_optimizer = popt(self.target_policy)
        self.qf_optimizers = []
        for k, qf in enumerate(self.qfs):
            frozen_k = frozen[k] if self.unshared else not self.train_bias
            q_no_grad = [i for i, (n, _) in enumerate(qf.named_parameters())
                         if n == "last_fc.bias"] if frozen_k else []
            self.qf_optimizers.append(AdamStateView(
                self, list(qf.parameters()), tw(self.adam_m, qf), tw(self.adam_v, qf),
                qf_lr[k] if self.unshared else qf_lr, (0.9, 0.999), 1e-8, no_grad=q_no_grad))
        # SACTrainer's alpha (snapshot keys only)
        self.alpha_optimizer = AdamStateView(self, [self.log_alpha], [self.alpha_state[1:2]],
                                             [self.alpha_state[2:3]], policy_lr, (0.9, 0.999),
                                             1e-8)
        self.eval_statistics = OrderedDict()
        self._n_train_steps_total = 0
        self._need_to_update_eval_statistics = True

    def _make_target_policy_network(self, policy_producer):
        """use_target_policy without mean_update (particle_trainer.py:150-154,
        gaussian_trainer.py:154-158): a policy_producer() network overwritten
        with a copy of the policy (soft update, tau 1) that supplies the next
        actions of the TD target (:196-199).  The reference's per-step soft
        update copies this network onto itself (:386-388 / :385-387), so it
        keeps the weights it has -- here a frozen block outside the Adam arena
        (oac_sac_buffers.next_policy), loadable like the reference's."""
        self.target_policy_network = None
        self._tpn = None
        if not (self.use_target_policy and not self.mean_update):
            return
        policy_producer()   # the reference's producer call (its init is overwritten)
        lay = self.layout
        self._tpn = self.params[:lay.pol_size].clone()
        self.target_policy_network = ArenaTanhGaussianPolicy(
            self._tpn, 0, lay, self.obs_dim, self.act_dim, self.hidden)

    def _next_policy_ptr(self):
        return None if getattr(self, "_tpn", None) is None else self._tpn.data_ptr()

    # ------------------------------------------------------------ global_opt
    def _make_init_policies(self, ref_init, ref_init_tp):
        """global_opt (gaussian_trainer.py:143-151, particle_trainer.py:139-144):
        ``init_policy`` / ``init_target_policy``, two policy_producer()
        networks that are never trained -- frozen policy-shaped blocks outside
        the Adam arena; like the reference's, neither in ``networks`` nor in
        the snapshot.  optimize_policies restarts the policy from init_policy."""
        self.policy_opt_history = None
        self._sweep = None
        if not self.global_opt:
            return
        if self.use_graph:
            raise NotImplementedError("global_opt with use_graph=True: a global_opt step is "
                                      "issued as direct launches; unsupported: ['use_graph']")
        lay = self.layout
        mods = []
        for ref in (ref_init, ref_init_tp):
            block = torch.zeros(int(lay.pol_size), dtype=torch.float32, device=self.device)
            mod = ArenaTanhGaussianPolicy(block, 0, lay, self.obs_dim, self.act_dim, self.hidden)
            mod.load_state_dict({k: v.detach() for k, v in ref.state_dict().items()})
            mods.append((block, mod))
        (self._init_pol, self.init_policy), (self._init_tpol, self.init_target_policy) = mods
        # the sweep's own counters (oac_sac_policy_opt_iter's opt_state): 64 bytes
        self._popt_state = torch.zeros(8, dtype=torch.int64, device=self.device)

    def _set_policy_opt_steps(self, n):
        self._policy_opt_steps = int(n)
        if self.global_opt:
            self._popt_state.zero_()
            self._popt_state[0] = self._policy_opt_steps

    _SWEEP_SLOTS = 32   # index ring slots (two completion chunks: staging runs 16 iterations ahead)

    def _sweep_rows(self, buffer):
        """(rows [>= N + 1, row_stride] on the device, N): the buffer's own
        device storage, or a get_dataset() array uploaded once.  One spare row
        behind the N lets shuffle='none' read the rows in place."""
        stride = self.rows["row_stride"]
        st = getattr(buffer, "_storage", None)
        if torch.is_tensor(st) and st.is_cuda and st.shape[1] == stride:
            N = int(buffer._size)
            if st.shape[0] > N:
                return st, N
            spare = torch.zeros(N + 1, stride, dtype=torch.float32, device=self.device)
            spare[:N].copy_(st[:N])
            return spare, N
        data = buffer.get_dataset()
        data = torch.as_tensor(np.asarray(data) if not torch.is_tensor(data) else data)
        N = int(data.shape[0])
        rows = torch.zeros(N + 1, stride, dtype=torch.float32, device=self.device)
        o = self.rows["off_obs"]
        rows[:N, o:o + self.obs_dim].copy_(data.reshape(N, self.obs_dim).to(torch.float32))
        return rows, N

    def _sweep_plan(self, rows, N):
        """The one sweep plan (batch = N): a new N or store replaces it."""
        key = (N, rows.data_ptr())
        if self._sweep is not None and self._sweep[0] == key:
            self._sweep[1].rows = rows
            return self._sweep[1]
        if self._sweep is not None:
            old = self._sweep[1]
            self._sweep = None
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            torch.cuda.synchronize(self.device)   # (its launches read its workspace)
            self._plans.pop(old.key, None)
            check(_lib.lib().oac_sac_destroy(old.handle))
        S = self._SWEEP_SLOTS
        ring = torch.zeros(S * N, dtype=torch.int32, device=self.device)
        plan = self._plan(N, replay=rows, idx=ring, ring_slots=S)
        check(_lib.lib().oac_sac_set_host_ring(plan.handle, None))
        plan.rings, plan.rows, plan.bc = (ring,), rows, 0
        self._sweep = (key, plan)
        return plan

    def optimize_policies(self, buffer, out_dir='', epoch=0, save_fig=False, *, iterations=150,
                          shuffle="reference"):
        """rl_algorithm.py:169-171 -> utils/core.py:64-137 optimize_policy: the
        policy restarts from ``init_policy`` and takes ``iterations`` Adam steps
        (its own optimizer: moments and step count carry on) on -mean(upper
        bound of the frozen critic) over the whole replay as one batch.
        shuffle='reference': each iteration's rows are what the reference's
        ``random.shuffle(dataset)`` leaves (shuffle_gather_indices; the global
        ``random`` stream advances exactly as there), staged while the GPU runs
        the previous iteration; 'none': rows 0..N-1 every iteration, no host
        work.  ``policy_opt_history`` = {'loss', 'grad_norm'} per iteration,
        read back once at the end."""
        if self.ensemble:   # particle_trainer.py:519-520
            return None
        if not self.global_opt:
            raise RuntimeError("optimize_policies needs a trainer built with global_opt=True")
        if save_fig:
            raise NotImplementedError("save_fig: plotting is out of scope; the curves are in "
                                      "trainer.policy_opt_history")
        if shuffle not in ("reference", "none"):
            raise ValueError(f"shuffle {shuffle!r}: 'reference' or 'none'")
        iterations = int(iterations)
        rows, N = self._sweep_rows(buffer)
        if N < 1 or iterations < 1:
            self.policy_opt_history = dict(loss=[], grad_norm=[])
            return None
        plan = self._sweep_plan(rows, N)
        hist = torch.zeros(iterations, 2, dtype=torch.float32, device=self.device)
        L = _lib.lib()
        opt = ctypes.c_void_p(self._popt_state.data_ptr())

        def go(sp):
            check(L.oac_sac_policy_opt_reset(plan.handle, ctypes.c_void_p(self._init_pol.data_ptr()),
                                             sp))
            idx = np.arange(N, dtype=np.int64)
            for k in range(iterations):
                row = ctypes.c_void_p(hist.data_ptr() + 8 * k)
                if shuffle == "none":
                    check(L.oac_sac_policy_opt_iter(plan.handle, None, 0, opt, row, sp))
                    continue
                idx = idx[shuffle_gather_indices(N)]
                check(L.oac_sac_policy_opt_iter(plan.handle, ctypes.c_void_p(idx.ctypes.data),
                                                plan.bc, opt, row, sp))
                plan.bc += 1
        self._on_stream(go)
        self._policy_opt_steps += iterations
        h = hist.cpu().numpy()
        self.policy_opt_history = dict(loss=h[:, 0].tolist(), grad_norm=h[:, 1].tolist())
        return None

    def _make_cfg(self, batch):
        c = super()._make_cfg(batch)
        c.std_soft_update = int(bool(self.std_soft_update))
        c.std_soft_prob = float(self.std_soft_update_prob)
        c.mean_update = int(bool(self.mean_update))
        c.freeze_q_bias = int(not self.train_bias)
        c.global_opt = int(bool(self.global_opt))
        c.unshared = int(bool(self.unshared))
        c.std_lr = float(self.std_lr or 0.0)
        return c

    @staticmethod
    def _stats(st, name, arr):
        """create_stats_ordered_dict (utils/eval_util.py) for one array."""
        st[name + " Mean"] = np.mean(arr)
        st[name + " Std"] = np.std(arr)
        st[name + " Max"] = np.max(arr)
        st[name + " Min"] = np.min(arr)

    def _tensor(self, x):
        return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x,
                               dtype=torch.float32, device=self.device)

    def get_diagnostics(self):
        return self.eval_statistics

    def end_epoch(self, epoch):
        self._need_to_update_eval_statistics = True

    @property
    def networks(self):
        # (particle_trainer.py:437-445: an ensemble lists its P policies)
        pols = list(self.policy.policies) if self.ensemble else [self.policy]
        nets = pols + self.qfs + self.tfs + [self.target_policy]
        if getattr(self, "target_policy_network", None) is not None:
            nets.append(self.target_policy_network)
        return nets

    def get_snapshot(self):
        """gaussian_trainer.py:452-482 / particle_trainer.py:449-478 (keys)."""
        d = dict(policy_state_dict=self.policy.state_dict(),
                    policy_optim_state_dict=self.policy_optimizer.state_dict(),
                    log_alpha=self.log_alpha,
                    alpha_optim_state_dict=self.alpha_optimizer.state_dict(),
                    eval_statistics=_plain_stats(self.eval_statistics),
                    _n_train_steps_total=self._n_train_steps_total,
                    _need_to_update_eval_statistics=self._need_to_update_eval_statistics,
                    qfs_state_dicts=[q.state_dict() for q in self.qfs],
                    qfs_optims_state_dicts=[o.state_dict() for o in self.qf_optimizers],
                    target_qfs_state_dicts=[t.state_dict() for t in self.tfs],
                    target_policy_state_dict=self.target_policy.state_dict(),
                    target_policy_opt_state_dict=self.target_policy_optimizer.state_dict())
        if getattr(self, "target_policy_network", None) is not None:
            d["target_policy_network"] = self.target_policy_network.state_dict()
        if self.ensemble:
            # policy_state_dict is the list of P state dicts and policy_optim_state_dict
            # the never-stepped parent optimizer, as the reference writes them; the P
            # optimizers it leaves out are an extra key
            d["policy_optims_state_dicts"] = [o.state_dict() for o in self.policy_optimizers]
        return d

    def restore_from_snapshot(self, ss):
        """gaussian_trainer.py:484-517 / particle_trainer.py:480-505."""
        self.policy.load_state_dict(ss["policy_state_dict"])
        self.policy_optimizer.load_state_dict(ss["policy_optim_state_dict"])
        if self.ensemble and "policy_optims_state_dicts" in ss:
            # (a reference-written snapshot has no such key: the moments stay as they are)
            for opt, sd in zip(self.policy_optimizers, ss["policy_optims_state_dicts"]):
                opt.load_state_dict(sd)
        if self.global_opt:   # the policy optimizer's own step count, back into the device counter
            steps = [int(v["step"]) for v in ss["policy_optim_state_dict"]["state"].values()]
            self._set_policy_opt_steps(max(steps) if steps else 0)
        for i in range(len(ss["qfs_state_dicts"])):
            self.qfs[i].load_state_dict(ss["qfs_state_dicts"][i])
            self.qf_optimizers[i].load_state_dict(ss["qfs_optims_state_dicts"][i])
            self.tfs[i].load_state_dict(ss["target_qfs_state_dicts"][i])
        self.log_alpha.copy_(torch.as_tensor(ss["log_alpha"]).reshape(1))
        self.alpha_optimizer.load_state_dict(ss["alpha_optim_state_dict"])
        self.eval_statistics = ss["eval_statistics"]
        self._n_train_steps_total = int(ss["_n_train_steps_total"])
        self._need_to_update_eval_statistics = ss["_need_to_update_eval_statistics"]
        self.target_policy.load_state_dict(ss["target_policy_state_dict"])
        self.target_policy_optimizer.load_state_dict(ss["target_policy_opt_state_dict"])
        if getattr(self, "target_policy_network", None) is not None:
            self.target_policy_network.load_state_dict(ss["target_policy_network"])
        self.step_state[0] = self._n_train_steps_total
