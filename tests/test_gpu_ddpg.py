"""GPU parity of oac_amd.DDPGTrainer (OAC_KIND_DDPG, csrc/ddpg_plan.hip)
against the reference's own outputs (tests/golden/ddpg_*.npz,
make_golden_ddpg.py) and the CPU restatement (tests/ddpg_oracle.py): the
torch-1.4 update order (policy gradient through the post-step critic with
the pre-step masks), the frozen target_policy_network, the drop-in call path,
both kernel sets, and the fixed-std policy."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ddpg_oracle as do
import parity
from gpu_helpers import Space, StateDictModule, module_tensors

pytestmark = pytest.mark.gpu

FIXTURES = ["ddpg_small", "ddpg_fixed_std", "ddpg_tpn", "ddpg_stress", "ddpg_humanoid"]
HERE = os.path.dirname(os.path.abspath(__file__))


class PolicyModule(StateDictModule):
    """What the reference's policy_producer returns, as far as DDPGTrainer
    reads it: state_dict() and the std attribute (policies.py:236)."""

    def __init__(self, sd, std):
        super().__init__(sd)
        self.std = std


def producers(params, std, act_dim):
    qs = iter([params["qf"], params["target_qf"]])
    std = None if std is None else np.ones(act_dim) * std
    return (lambda **k: PolicyModule(params["policy"], std),
            lambda **k: StateDictModule(next(qs)))


def trainer_for(meta, g=None, params=None, **kw):
    from oac_amd import DDPGTrainer
    params = params or do.params_of(meta)
    pp, qp = producers(params, meta["std"], meta["act_dim"])
    tr = DDPGTrainer(pp, qp, action_space=Space(meta["act_dim"]), discount=meta["discount"],
                     reward_scale=meta["reward_scale"], policy_lr=meta["lr"], qf_lr=meta["lr"],
                     soft_target_tau=meta["tau"], target_update_period=meta["period"],
                     use_target_policy=meta["use_target_policy"], **kw)
    tpn = do.next_policy_of(g) if g is not None else None
    if tpn:   # the fixture's own target_policy_network weights
        tr.target_policy_network.load_state_dict({k: torch.as_tensor(v) for k, v in tpn.items()})
    return tr


def step_errors(tr, g, s, lr):
    """{golden key: error} of the trainer's state after step s: gradients,
    post-step parameters and target critic (whole tensors), statistics."""
    errs = {}
    for grp, mod in (("policy", tr.policy), ("qf", tr.qf)):
        gv = module_tensors(tr, mod, tr.grads)
        for pn in gv:
            key = f"s{s}/grad/{grp}/{pn}"
            errs[key] = parity.compare(g, key, gv[pn].cpu().numpy())
    for grp, mod in (("policy", tr.policy), ("qf", tr.qf), ("tf", tr.target_qf)):
        for pn, t in mod.state_dict().items():
            key = f"s{s}/post/{grp}/{pn}"
            gk = f"s{s}/grad/{grp}/{pn}" if s == 0 and grp != "tf" else None
            errs[key], _ = parity.compare_post(g, key, gk, t.cpu().numpy(), lr)
    for k, v in tr.get_diagnostics().items():
        errs[f"s{s}/stat/{k}"] = parity.stat_err(v, g, f"s{s}/stat/{k}")
    return errs


def gated(errs, noise):
    return {k: (v, noise[k]) for k, v in errs.items() if v > parity.gate(k, noise[k])}


@pytest.mark.parametrize("name", FIXTURES)
def test_ddpg_step_matches_reference_golden(name):
    meta, g = parity.load(name)
    tr = trainer_for(meta, g)
    errs = {}
    for s in range(meta["steps"]):
        tr.end_epoch(s)
        tr.train_from_torch(do.batch_of(meta, g[f"s{s}/idx"]))
        torch.cuda.synchronize()
        errs.update(step_errors(tr, g, s, meta["lr"]))
    assert set(errs) == do.golden_keys(g)
    bad = gated(errs, do.noise_of(meta, g))
    print(name, "worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


def test_ddpg_stats_and_snapshot_keys():
    meta, g = parity.load("ddpg_small")
    tr = trainer_for(meta, g)
    tr.train_from_torch(do.batch_of(meta, g["s0/idx"]))
    keys = [k[len("s0/stat/"):] for k in g if k.startswith("s0/stat/")]
    assert list(tr.get_diagnostics().keys()) == keys
    base = {"policy_state_dict", "policy_optim_state_dict", "qf_state_dict", "qf_optim_state_dict",
            "target_qf_state_dict", "eval_statistics", "_n_train_steps_total",
            "_need_to_update_eval_statistics"}                  # ddpg_trainer.py:204-213
    assert set(tr.get_snapshot()) == base
    meta2, g2 = parity.load("ddpg_tpn")
    tr2 = trainer_for(meta2, g2)
    assert set(tr2.get_snapshot()) == base | {"target_policy_network"}   # :214-215
    assert len(tr2.networks) == 4 and len(tr.networks) == 3


def test_ddpg_log_std_head_untouched():
    """ddpg_small's policy has a log-std head: the deterministic step gives it
    no gradient, Adam leaves it bit-identical and keeps no state for it."""
    meta, g = parity.load("ddpg_small")
    tr = trainer_for(meta, g)
    before = {k: v.clone() for k, v in tr.policy.state_dict().items()}
    for s in range(2):
        tr.train_from_torch(do.batch_of(meta, g[f"s{s}/idx"]))
    torch.cuda.synchronize()
    after = tr.policy.state_dict()
    for k in do.LOG_STD_KEYS:
        assert torch.equal(before[k], after[k]), k
    assert not torch.equal(before["last_fc.weight"], after["last_fc.weight"])
    assert sorted(tr.get_snapshot()["policy_optim_state_dict"]["state"]) == [0, 1, 2, 3, 4, 5]


def test_ddpg_frozen_target_network_and_update_period():
    meta, g = parity.load("ddpg_tpn")
    assert meta["period"] == 2
    tr = trainer_for(meta, g)
    loaded = {k: v.clone() for k, v in tr.target_policy_network.state_dict().items()}
    assert not torch.equal(loaded["fc0.weight"], tr.policy.state_dict()["fc0.weight"])
    tf = []
    for s in range(meta["steps"]):
        tr.train_from_torch(do.batch_of(meta, g[f"s{s}/idx"]))
        torch.cuda.synchronize()
        tf.append({k: v.clone() for k, v in tr.target_qf.state_dict().items()})
    for k, v in tr.target_policy_network.state_dict().items():
        assert torch.equal(v, loaded[k]), k
    for k in tf[0]:   # n = 1: no soft update; n = 2: one
        assert torch.equal(tf[0][k], tf[1][k]), k
    assert not torch.equal(tf[1]["fc0.weight"], tf[2]["fc0.weight"])


def test_ddpg_reference_snapshot_restores_and_resumes():
    fx = torch.load(os.path.join(HERE, "golden", "ddpg_snapshot.pt"), weights_only=True)
    meta = fx["meta"]
    tr = trainer_for(meta)
    tr.restore_from_snapshot(fx["snapshot"])
    assert tr._n_train_steps_total == 2
    tr.end_epoch(2)
    batch = do.batch_of(meta, fx["step3"]["idx"].numpy())
    tr.train_from_torch(batch)
    torch.cuda.synchronize()
    assert tr._n_train_steps_total == 3
    assert int(tr.step_state[0].item()) == 3          # Adam's t continued from the restored count
    st = tr.get_snapshot()["policy_optim_state_dict"]["state"]
    assert all(v["step"] == 3 for v in st.values())
    # the gate: the reference's own fp32 distance from the float64 oracle run
    # through the same three steps
    idx = [i.numpy() for i in fx["pre_idx"]] + [fx["step3"]["idx"].numpy()]
    o64 = do.make_oracle(meta, dtype=torch.float64)
    for i in idx:
        o64.step(do.batch_of(meta, i))
    bad = {}
    for grp, mod, orc in (("policy", tr.policy, o64.P), ("qf", tr.qf, o64.Q),
                          ("tf", tr.target_qf, o64.T)):
        for pn, t in mod.state_dict().items():
            ref = fx["step3"]["post"][grp][pn].numpy()
            noise = parity.rel_err(orc[pn].numpy(), ref)
            e = parity.rel_err(t.cpu().numpy(), ref)
            if e > parity.gate(pn, noise):
                bad[f"{grp}/{pn}"] = (e, noise)
    assert not bad, bad
    # and the snapshot it writes itself loads with weights_only=True
    import io
    buf = io.BytesIO()
    torch.save(tr.get_snapshot(), buf)
    buf.seek(0)
    ss = torch.load(buf, weights_only=True)
    assert set(ss["target_policy_network"]) == set(do.POLICY_KEYS)


def test_ddpg_dropin_path_matches_reference_golden():
    """rl_algorithm.py:160-167 as the reference runs it: random_batch on
    numpy's global stream, then train(batch) -- oac_sac_step_host_idx -- at the
    recipe's shape.  The drawn indices are the golden's; same gates."""
    from oac_amd import ReplayBuffer
    from fixtures_lib import synthetic_transitions
    meta, g = parity.load("ddpg_humanoid")
    tr = trainer_for(meta, g)
    n = meta["n_replay"]
    rb = ReplayBuffer(n, Space(meta["obs_dim"]), Space(meta["act_dim"]), device="cuda:0")
    d = synthetic_transitions(n, meta["obs_dim"], meta["act_dim"], seed=0)
    rb.add_paths([dict(observations=d["observations"], actions=d["actions"], rewards=d["rewards"],
                       next_observations=d["next_observations"], terminals=d["terminals"])])
    np.random.seed(meta["idx_seed"])
    errs = {}
    for s in range(meta["steps"]):
        tr.end_epoch(s)
        batch = rb.random_batch(meta["B"])
        assert np.array_equal(batch.host_indices, g[f"s{s}/idx"])
        batch["buffer"] = rb
        tr.train(batch)
        torch.cuda.synchronize()
        plan = tr._last_plan
        assert plan is tr._dropin[(meta["B"], rb._storage.data_ptr())], "not the drop-in plan"
        row = rb._storage.shape[1]
        rows = rb._storage[torch.as_tensor(g[f"s{s}/idx"], device=rb._storage.device)]
        assert torch.equal(plan.views["batch"][:, :row], rows), "in-step gather differs from the replay rows"
        errs.update(step_errors(tr, g, s, meta["lr"]))
    bad = gated(errs, do.noise_of(meta, g))
    print("dropin worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]
    # the recipe's step form: rows read through the host index slot by the
    # layer-0 launch (no gather launch), fused Adam, 10 launches
    from oac_amd._lib import TRACE, lib
    bits = lib().oac_sac_trace(plan.handle, 1)
    assert bits & TRACE["direct"] and bits & TRACE["fused"], bits
    assert lib().oac_sac_launch_count(plan.handle) == 10


def _oracle_step_check(meta, B, seed):
    """One step from the fixture-style initial state on a random batch against
    the float32 oracle on the same inputs: 1e-5 per gradient tensor."""
    params = do.params_of(meta)
    tr = trainer_for(meta, params=params)
    rs = np.random.RandomState(seed)
    b = do.batch_of(meta, rs.randint(0, meta["n_replay"], B))
    tr.train_from_torch(b)
    torch.cuda.synchronize()
    out = do.make_oracle(meta).step(b)
    worst = {}
    for grp, mod in (("policy", tr.policy), ("qf", tr.qf)):
        gv = module_tensors(tr, mod, tr.grads)
        for pn, ref in out["grads"][grp].items():
            worst[f"{grp}/{pn}"] = parity.rel_err(gv[pn].cpu().numpy(), ref.numpy())
    v = tr._last_plan.views
    for name, ref in (("q1", out["q_pred"]), ("qnew", out["q_new"]), ("tq1", out["tq"]),
                      ("y", out["q_target"]), ("act1", out["act"]), ("act2", out["next_act"])):
        worst[f"view/{name}"] = parity.rel_err(v[name].cpu().numpy(), ref.numpy())
    print(B, sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    bad = {k: e for k, e in worst.items() if e > 1e-5}
    assert not bad, bad
    return tr


def test_ddpg_large_batch_kernel_set_matches_oracle():
    """B = 1024 is the smallest batch that selects the large-batch kernel set."""
    meta = dict(obs_dim=376, act_dim=17, hidden=[256, 256], seed=5, std=0.1, pi_init_w=1e-3,
                q_init_w=3e-3, discount=0.99, reward_scale=1.0, tau=1e-2, lr=1e-3, period=1,
                use_target_policy=True, n_replay=20000)
    tr = _oracle_step_check(meta, 1024, 1024)
    from oac_amd._lib import TRACE, lib
    assert not lib().oac_sac_trace(tr._last_plan.handle, 0) & TRACE["fused"]


@pytest.mark.parametrize("B", [40, 520])
def test_ddpg_ragged_batch_matches_oracle(B):
    """B = 40: no multiple of the 16-row blocks or the 32-row tiles, more than
    one block; the fused step with the shadow weights.  B = 520: the
    small-batch kernel set with split-K weight gradients (512 <= B < 1024), so
    no fused Adam and no shadow -- the Adam launches and the unmerged
    -mean(q_new) backward on the small kernels."""
    meta = dict(obs_dim=11, act_dim=3, hidden=[16, 16], seed=9, std=0.1, pi_init_w=0.5,
                q_init_w=0.5, discount=0.99, reward_scale=1.0, tau=1e-2, lr=1e-3, period=1,
                use_target_policy=False, n_replay=200 if B == 40 else 2000)
    tr = _oracle_step_check(meta, B, B)
    from oac_amd._lib import TRACE, lib
    assert bool(lib().oac_sac_trace(tr._last_plan.handle, 0) & TRACE["fused"]) == (B == 40)


def test_ddpg_launch_count():
    """The step's launches (oac_sac_launch_count) at the recipe's shape with
    the batch given: 10, the SAC step's count at this shape."""
    from oac_amd._lib import lib
    meta, g = parity.load("ddpg_humanoid")
    tr = trainer_for(meta, g)
    tr.train_from_torch(do.batch_of(meta, g["s0/idx"]))
    torch.cuda.synchronize()
    assert lib().oac_sac_launch_count(tr._last_plan.handle) == 10


def test_fixed_std_policy_forward_and_rollout():
    """ArenaTanhGaussianPolicy(std=...): the reference's 6-tuple
    (policies.py:260-316 with :280-282) against a float64 restatement at 1e-6
    absolute, deterministic and sampled; six state_dict keys;
    MakeDeterministic and vec_rollout run over it."""
    from oac_amd import MakeDeterministic, vec_rollout
    from test_rollout import ToyEnv
    meta, g = parity.load("ddpg_fixed_std")
    tr = trainer_for(meta, g)
    pol = tr.policy
    assert list(pol.state_dict()) == do.POLICY_KEYS
    Do, Da = meta["obs_dim"], meta["act_dim"]
    obs = np.random.RandomState(3).standard_normal((64, Do)).astype(np.float32)
    P = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in do.params_of(meta)["policy"].items()}
    mean64 = do.det_forward(torch.as_tensor(obs, dtype=torch.float64), P)["mean"].numpy()
    std64 = np.full(Da, 0.1)

    def close(got, ref, what):
        got = got.detach().cpu().numpy().astype(np.float64)
        assert got.shape == np.shape(ref), (what, got.shape, np.shape(ref))
        assert np.max(np.abs(got - ref)) <= 1e-6, (what, np.max(np.abs(got - ref)))

    a, mean, log_std, log_prob, std, pre = pol(torch.as_tensor(obs), deterministic=True)
    close(a, np.tanh(mean64), "action")
    close(mean, mean64, "mean")
    close(log_std, np.log(std64), "log_std")
    close(std, std64, "std")
    close(pre, mean64, "pre_tanh")
    close(log_prob, np.zeros((64, Da)), "log_prob")

    torch.manual_seed(11)
    a, mean, log_std, log_prob, std, pre = pol(torch.as_tensor(obs), return_log_prob=True)
    torch.manual_seed(11)
    eps = torch.randn(64, Da, device=a.device).cpu().numpy().astype(np.float64)
    z = mean64 + std64 * eps
    lp = (-(z - mean64) ** 2 / (2 * std64 ** 2) - np.log(std64) - np.log(np.sqrt(2 * np.pi))
          - np.log(1 - np.tanh(z) ** 2 + 1e-6)).sum(1, keepdims=True)
    close(a, np.tanh(z), "action")
    close(mean, mean64, "mean")
    close(log_std, np.log(std64), "log_std")
    close(std, std64, "std")
    close(pre, z, "pre_tanh")
    close(log_prob, lp, "log_prob")
    assert np.std(a.cpu().numpy() - np.tanh(mean64)) > 0.01   # the call did sample

    det = MakeDeterministic(pol)
    one, _ = det.get_action(obs[0])
    assert np.max(np.abs(one - np.tanh(mean64[0]))) <= 1e-6
    for agent in (det, pol):
        paths = vec_rollout([ToyEnv(Do, L, s) for s, L in enumerate((3, 5))], agent,
                            max_path_length=4)
        assert [len(p["actions"]) for p in paths] == [3, 4]
        assert all(np.all(np.isfinite(p["actions"])) for p in paths)


def test_ddpg_data_parallel_entry_points_name_the_kind():
    from oac_amd import _lib
    meta, g = parity.load("ddpg_fixed_std")
    tr = trainer_for(meta, g)
    tr.train_from_torch(do.batch_of(meta, g["s0/idx"]))
    torch.cuda.synchronize()
    L, h = _lib.lib(), tr._last_plan.handle
    s = _lib.stream_ptr(tr.stream)
    assert L.oac_sac_step_phase(h, 0, 0, s) != 0
    msg = L.oac_last_error()
    assert b"DDPG" in msg and b"kind 4" in msg, msg
    hook = _lib.ALLREDUCE_FN(lambda ctx, buf, n, stream: 0)
    assert L.oac_sac_set_allreduce(h, ctypes.cast(hook, ctypes.c_void_p), None, 0) != 0
    msg = L.oac_last_error()
    assert b"DDPG" in msg and b"kind 4" in msg, msg
    assert L.oac_sac_set_step_graph(h, None, 0) != 0
    assert b"DDPG" in L.oac_last_error()
    assert L.oac_sac_step(h, _lib.OAC_STEP_USE_GRAPH, s) != 0     # rejected, not ignored
    msg = L.oac_last_error()
    assert b"DDPG" in msg and b"GRAPH" in msg, msg
    before = tr.policy.state_dict()["fc0.weight"].clone()
    torch.cuda.synchronize()
    assert torch.equal(before, tr.policy.state_dict()["fc0.weight"])   # none of them stepped
