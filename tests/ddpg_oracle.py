"""CPU restatement of the reference DDPGTrainer step
(/root/reference/trainer/ddpg_trainer.py:92-184) in float32 or float64, from
the building blocks of oracle.sac_oracle, and the shared inputs of the DDPG
fixtures (tests/golden/make_golden_ddpg.py runs the reference on them).

Per step, n = steps taken so far:
  a~ = tanh(mean_pi(obs)), q_new = Q(obs, a~), q_pred = Q(obs, act): pre-step
  a' = tanh(mean_nu(next_obs)) (nu = the policy, or the frozen
  target_policy_network), y = scale r + (1 - d) gamma Q_T(next_obs, a')
  critic: grad of mean((q_pred - y)^2), Adam at t = n + 1
  policy: grad of -mean(q_new) through the critic graph with the POST-step
  critic weights and the PRE-step activations / masks (torch 1.4 steps through
  p.data, so backward() after the critic's step sees the new weights: SURVEY
  quirk Q1), times (1 - a~^2), through the pre-step policy; Adam
  n % period == 0: target critic <- tau Q_post + (1 - tau) target critic
``quirk=False`` sends the policy gradient through the pre-step critic instead
(what an implementation that ignores the ordering computes).
"""
import numpy as np
import torch

from fixtures_lib import mlp_params
from oracle import sac_oracle as so

POLICY_KEYS = ["fc0.weight", "fc0.bias", "fc1.weight", "fc1.bias", "last_fc.weight", "last_fc.bias"]
LOG_STD_KEYS = ["last_fc_log_std.weight", "last_fc_log_std.bias"]
STAT_KEYS = (["QF mean", "Q Loss", "Policy Loss"] +
             [f"{n} {s}" for n in ("Q Predictions", "Q Targets", "Policy mu")
              for s in ("Mean", "Std", "Max", "Min")])


def ddpg_params(obs_dim, act_dim, hidden, seed, pi_init_w=1e-3, q_init_w=3e-3, log_std_head=False):
    """policy, qf, target_qf and the target_policy_network's own weights (fp32)."""
    rs = np.random.RandomState(seed)
    pol = mlp_params(rs, obs_dim, hidden, act_dim, pi_init_w, log_std_head=log_std_head)
    qf = mlp_params(rs, obs_dim + act_dim, hidden, 1, q_init_w)
    tf = mlp_params(rs, obs_dim + act_dim, hidden, 1, q_init_w)
    rs2 = np.random.RandomState(seed + 100)
    tpn = mlp_params(rs2, obs_dim, hidden, act_dim, pi_init_w, log_std_head=log_std_head)
    return dict(policy=pol, qf=qf, target_qf=tf, tpn=tpn)


def params_of(meta):
    return ddpg_params(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["seed"],
                       pi_init_w=meta["pi_init_w"], q_init_w=meta["q_init_w"],
                       log_std_head=meta["std"] is None)


def det_forward(obs, p):
    """TanhGaussianPolicy.forward(deterministic=True), policies.py:272-288."""
    hs = so.mlp_trunk(obs, p)
    mean = so.linear(hs[-1], p["last_fc.weight"], p["last_fc.bias"])
    return dict(hs=hs, mean=mean, a=torch.tanh(mean))


def det_backward(c, p, ga):
    """Gradient of sum(ga * tanh(mean)) w.r.t. the policy's parameters; a
    log-std head (unused by the deterministic forward) gets zeros."""
    a, hs = c["a"], c["hs"]
    dmean = ga * (1 - a * a)
    L = len(hs) - 1
    g = {"last_fc.weight": dmean.t() @ hs[L], "last_fc.bias": dmean.sum(0)}
    for k in LOG_STD_KEYS:
        if k in p:
            g[k] = torch.zeros_like(p[k])
    dh = (dmean @ p["last_fc.weight"]) * (hs[L] > 0)
    for i in range(L - 1, -1, -1):
        g[f"fc{i}.weight"] = dh.t() @ hs[i]
        g[f"fc{i}.bias"] = dh.sum(0)
        if i > 0:
            dh = (dh @ p[f"fc{i}.weight"]) * (hs[i] > 0)
    return g


class DDPGOracle:
    def __init__(self, params, obs_dim, act_dim, discount=0.99, reward_scale=1.0, policy_lr=1e-3,
                 qf_lr=1e-3, tau=1e-2, target_update_period=1, next_policy=None,
                 dtype=torch.float32, quirk=True):
        self.dtype, self.Do, self.Da = dtype, obs_dim, act_dim
        self.P = so.to_torch_params(params["policy"], dtype)
        self.Q = so.to_torch_params(params["qf"], dtype)
        self.T = so.to_torch_params(params["target_qf"], dtype)
        self.NP = None if next_policy is None else so.to_torch_params(next_policy, dtype)
        self.discount, self.reward_scale, self.tau = discount, reward_scale, tau
        self.period, self.quirk = target_update_period, quirk
        self.opt_p = so.Adam14(self.P, policy_lr)
        self.opt_q = so.Adam14(self.Q, qf_lr)
        self.n_steps = 0

    def step(self, batch):
        dt = self.dtype
        obs, act = so._t(batch["observations"], dt), so._t(batch["actions"], dt)
        rew, term = so._t(batch["rewards"], dt), so._t(batch["terminals"], dt)
        nobs = so._t(batch["next_observations"], dt)
        B = obs.shape[0]
        pf = det_forward(obs, self.P)                                    # :102-104
        cn = so.q_forward(obs, pf["a"], self.Q)                          # :106
        c = so.q_forward(obs, act, self.Q)                               # :114
        pf2 = det_forward(nobs, self.NP if self.NP is not None else self.P)   # :117-125
        tq = so.q_forward(nobs, pf2["a"], self.T)["q"]                   # :127
        y = self.reward_scale * rew + (1. - term) * self.discount * tq   # :129-130
        q_loss = ((c["q"] - y) ** 2).mean()                              # :132
        gq = so.q_param_grads(c, 2.0 * (c["q"] - y) / B, self.Q)
        q_pre = {k: v.clone() for k, v in self.Q.items()}
        self.opt_q.step(gq)                                              # :136-138
        g0 = -torch.ones_like(cn["q"]) / B                               # :108, :140-141
        da = so.q_input_grad(cn, g0, self.Q if self.quirk else q_pre)[:, self.Do:]
        gp = det_backward(pf, self.P, da)
        self.opt_p.step(gp)                                              # :142
        if self.n_steps % self.period == 0:                              # :147-151
            so.polyak(self.T, self.Q, self.tau)
        self.n_steps += 1
        self.last = dict(grads=dict(policy=gp, qf=gq), q_pred=c["q"], q_target=y, q_new=cn["q"],
                         q_loss=q_loss, mean=pf["mean"], tq=tq, act=pf["a"], next_act=pf2["a"])
        return self.last


def ddpg_stats(out):
    """ddpg_trainer.py:166-183, in its key order."""
    def np64(t):
        return np.asarray(t.detach().numpy(), np.float64)
    st = {"QF mean": np64(out["q_pred"]).mean(), "Q Loss": float(out["q_loss"]),
          "Policy Loss": float((-out["q_new"]).mean())}
    for name, x in (("Q Predictions", out["q_pred"]), ("Q Targets", out["q_target"]),
                    ("Policy mu", out["mean"])):
        x = np64(x)
        st.update({f"{name} Mean": x.mean(), f"{name} Std": x.std(), f"{name} Max": x.max(),
                   f"{name} Min": x.min()})
    return st


def next_policy_of(g):
    tpn = {k[4:]: v for k, v in g.items() if k.startswith("tpn/")}
    return tpn or None


def make_oracle(meta, g=None, dtype=torch.float32, quirk=True):
    """use_target_policy: the frozen network holds the fixture's recorded
    weights (tpn/*), or -- none recorded -- the copy of the initial policy the
    constructor makes (ddpg_trainer.py:66-70)."""
    params = params_of(meta)
    nxt = None
    if meta["use_target_policy"]:
        nxt = (next_policy_of(g) if g is not None else None) or params["policy"]
    return DDPGOracle(params, meta["obs_dim"], meta["act_dim"], discount=meta["discount"],
                      reward_scale=meta["reward_scale"], policy_lr=meta["lr"], qf_lr=meta["lr"],
                      tau=meta["tau"], target_update_period=meta["period"], next_policy=nxt,
                      dtype=dtype, quirk=quirk)


def batch_of(meta, idx):
    from fixtures_lib import synthetic_transitions
    tr = synthetic_transitions(meta["n_replay"], meta["obs_dim"], meta["act_dim"], seed=0)
    return {k: v[idx] for k, v in tr.items()}


def golden_keys(g):
    """The compared entries of a fixture: every gradient, post-step parameter
    and statistic (sampled tensors under their base key)."""
    keys = set()
    for k in g:
        if "/grad/" in k or "/post/" in k or "/stat/" in k:
            keys.add(k.split("#")[0])
    return keys


def oracle_errors(meta, g, orc):
    """{golden key: error} of the oracle run through the fixture's steps --
    every gradient and post-step tensor whole (no row left out), every
    statistic."""
    import parity
    errs = {}
    for s in range(meta["steps"]):
        out = orc.step(batch_of(meta, g[f"s{s}/idx"]))
        for grp in ("policy", "qf"):
            for pn, t in out["grads"][grp].items():
                key = f"s{s}/grad/{grp}/{pn}"
                errs[key] = parity.compare(g, key, t.numpy())
        for grp, params_ in (("policy", orc.P), ("qf", orc.Q), ("tf", orc.T)):
            for pn, t in params_.items():
                key = f"s{s}/post/{grp}/{pn}"
                gk = f"s{s}/grad/{grp}/{pn}" if s == 0 and grp != "tf" else None
                errs[key], _ = parity.compare_post(g, key, gk, t.numpy(), meta["lr"])
        st = ddpg_stats(out)
        for name, v in st.items():
            key = f"s{s}/stat/{name}"
            errs[key] = parity.stat_err(v, g, key)
    return errs


def noise_of(meta, g):
    """The reference's own fp32 distance from the float64 oracle, per key."""
    return oracle_errors(meta, g, make_oracle(meta, g, torch.float64))
