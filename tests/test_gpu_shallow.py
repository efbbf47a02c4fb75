"""One-hidden-layer networks (``--num_layers 1``, the riverswim recipes) for
the g-oac GaussianTrainer and the p-oac ParticleTrainer on the GPU: the
depth-1 step (csrc/det_plan.hip) against the reference's own runs
(tests/golden/*_d1_*.npz) and the CPU oracle, its launch count, the row-wise
evaluation kernels, snapshots and the entry paths."""
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity
import shallow_lib as sl
import test_oracle_golden as tog
from fixtures_lib import synthetic_transitions
from gpu_helpers import Space, StateDictModule, batch_from, module_tensors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


# ----------------------------------------------------------- golden parity
@pytest.mark.parametrize("name", sl.FIXTURES)
def test_step_matches_reference_golden(name):
    """Every gradient, post-step parameter and target, and the statistics
    (keys in the reference's order), at every step, under the project's gate;
    the log-std heads stay bit-untouched."""
    meta, g = parity.load(name)
    tr = sl.trainer_for(meta)
    assert tr.n_hidden == 1
    if meta.get("use_target_policy"):
        sl.load_tpn(tr, g)
    qf, tf = sl.critic_of(tr)
    pol_order, q_order = sl.orders(1)
    assert list(tr.policy.state_dict()) == pol_order and list(qf.state_dict()) == q_order
    heads0 = {(m, k): getattr(tr, m).state_dict()[k].clone()
              for m in ("policy", "target_policy") for k in pol_order[-2:]}
    errs = {}
    for s in range(meta["steps"]):
        tr.end_epoch(s)
        b = batch_from(meta, g[f"s{s}/idx"])
        if meta["counts"]:
            b["counts"] = g[f"s{s}/counts"][:, None]
        tr.train_from_torch(b)
        torch.cuda.synchronize()
        for grp, mod, order in (("policy", tr.policy, pol_order),
                                ("target_policy", tr.target_policy, pol_order),
                                ("qf", qf, q_order)):
            gv = module_tensors(tr, mod, tr.grads)
            for pn in order:
                key = f"s{s}/grad/{grp}/{pn}"
                errs[key] = parity.compare(g, key, gv[pn].cpu().numpy())
        for grp, mod in (("policy", tr.policy), ("target_policy", tr.target_policy),
                         ("qf", qf), ("tf", tf)):
            for pn, t in mod.state_dict().items():
                key = f"s{s}/post/{grp}/{pn}"
                gk = f"s{s}/grad/{grp}/{pn}" if s == 0 and grp != "tf" else None
                errs[key], _ = parity.compare_post(g, key, gk, t.cpu().numpy(), meta["lr"])
        keys = [k[len(f"s{s}/stat/"):] for k in g if k.startswith(f"s{s}/stat/")]
        assert list(tr.get_diagnostics().keys()) == keys
        for k, v in tr.get_diagnostics().items():
            errs[f"s{s}/stat/{k}"] = parity.stat_err(v, g, f"s{s}/stat/{k}")
    for (m, k), v in heads0.items():
        assert torch.equal(v, getattr(tr, m).state_dict()[k]), (m, k)
    noise = sl.oracle_errors(meta, g, torch.float64)
    bad = tog.gated(errs, noise)
    print(name, "worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]
    # Adam state as torch keeps it: none for the log-std heads (never a gradient)
    assert sorted(tr.policy_optimizer.state_dict()["state"]) == [0, 1, 2, 3]
    assert sorted(tr.target_policy_optimizer.state_dict()["state"]) == [0, 1, 2, 3]
    want_q = [0, 1, 2, 3] if meta["train_bias"] else [0, 1, 2]
    assert sorted(tr.qf_optimizers[0].state_dict()["state"]) == want_q


# ------------------------------------------------------- oracle, ragged
def _meta(kind, Do, Da, hidden, K=2, **kw):
    m = dict(kind=kind, obs_dim=Do, act_dim=Da, hidden=hidden, K=K, seed=3, q_min=0.0,
             q_max=50.0, pi_init_w=0.2, q_init_w=0.1, discount=0.99, delta=0.95, lr=3e-4,
             tau=5e-3, counts=True)
    m.update(kw)
    return m


def _batch(Do, Da, B, seed):
    data = synthetic_transitions(max(4 * B, 64), Do, Da, seed=seed)
    idx = np.random.RandomState(seed).randint(0, len(data["rewards"]), B)
    b = {k: v[idx] for k, v in data.items()}
    b["counts"] = np.random.RandomState(seed + 1).randint(0, 2, (B, 1)).astype(np.float64)
    return b


def _one_step_against_oracle(meta, B):
    """One step from identical state: every gradient tensor within 1e-5
    (norm-relative) of the fp32 CPU oracle's, as test_gpu_ragged.py."""
    params = sl.params_of(meta)
    tr = sl.trainer_for(meta, params=params)
    if meta["kind"] == "ptrain":
        meta = dict(meta, delta_index=tr.delta_index)
    b = _batch(meta["obs_dim"], meta["act_dim"], B, 6)
    tr.train_from_torch(b)
    torch.cuda.synchronize()
    pol_order, q_order = sl.orders(len(meta["hidden"]))
    out = sl.make_oracle(meta, params=params).step(b)
    worst = {}
    for grp, mod, order in (("policy", tr.policy, pol_order[:-2]),
                            ("target_policy", tr.target_policy, pol_order[:-2]),
                            ("qf", tr.qfs[0], q_order)):
        gv = module_tensors(tr, mod, tr.grads)
        for pn in order:
            worst[f"{grp}/{pn}"] = parity.rel_err(gv[pn].cpu().numpy(),
                                                  out["grads"][grp][pn].numpy())
    # the post-step parameters and the Polyak target (parity.compare_post: Adam's
    # first step is ~lr sign(g), so elements with a gradient at rounding level
    # are bounded separately)
    orc = sl.make_oracle(meta, params=params)
    out = orc.step(b)
    for grp, mod, want in (("policy", tr.policy, orc.P), ("target_policy", tr.target_policy, orc.TP),
                           ("qf", tr.qfs[0], orc.Q), ("tf", tr.tfs[0], orc.T)):
        for pn, t in mod.state_dict().items():
            gold = {"p": want[pn].numpy()}
            if grp != "tf":
                gold["g"] = out["grads"][grp][pn].numpy()
            worst[f"post/{grp}/{pn}"], _ = parity.compare_post(
                gold, "p", "g" if grp != "tf" else None, t.cpu().numpy(), meta["lr"])
    print(meta["kind"], meta["hidden"], B, sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    bad = {k: v for k, v in worst.items() if v > 1e-5}
    assert not bad, bad
    return tr


# (Do, Da, H, B): B = 1100 runs the large-batch kernel set and the unfused Adam,
# B = 600 the small-batch kernels with split-K slabs (unfused Adam too)
SHAPES = [(1, 1, 16, 1), (1, 1, 16, 32), (5, 2, 24, 37), (7, 5, 48, 300), (5, 2, 24, 1100),
          (5, 2, 24, 600)]
# the particle critic's K: 10 at B = 37, 2 and 16 at B = 32
RAGGED = [("goac",) + s + (2,) for s in SHAPES] + \
         [("ptrain",) + s + (k,) for s, k in zip(SHAPES, (5, 2, 10, 5, 5, 5))] + \
         [("ptrain", 1, 1, 16, 32, 16)]


@pytest.mark.parametrize("kind,Do,Da,H,B,K", RAGGED)
def test_depth_1_ragged(kind, Do, Da, H, B, K):
    tr = _one_step_against_oracle(_meta(kind, Do, Da, [H], K=K), B)
    assert tr.n_hidden == 1


@pytest.mark.parametrize("kind,K", [("goac", 2), ("ptrain", 10)])
def test_two_layers_at_the_riverswim_widths(kind, K):
    """(1, 1, 16, 32) with two hidden layers: the layer-0 launches the depth-1
    chain shares (inner dimension 1, act_dim 1, the [2, H] head matrix)."""
    tr = _one_step_against_oracle(_meta(kind, 1, 1, [16, 16], K=K), 32)
    assert tr.n_hidden == 2


# ---------------------------------------------------------- launch count
def _launches(tr):
    from oac_amd import _lib
    return _lib.lib().oac_sac_launch_count(tr._last_plan.handle)


@pytest.mark.parametrize("kind,K", [("goac", 2), ("ptrain", 10)])
def test_launch_count(kind, K):
    """Small batch, single process, batch given (no gather / counts launch):
    the depth-1 step takes at most 10 launches, fewer than two layers' 18."""
    n = {}
    for hidden in ([16], [16, 16]):
        meta = _meta(kind, 1, 1, hidden, K=K)
        tr = sl.trainer_for(meta)
        tr.train_from_torch(_batch(1, 1, 32, 6))
        torch.cuda.synchronize()
        n[len(hidden)] = _launches(tr)
    print(kind, n)
    assert n[2] == 18
    assert n[1] <= 10 and n[1] < n[2]
    assert n[1] == 8   # the count DESIGN.md records


# ----------------------------------------------------------- eval kernels
def _cpu_mlp(sd, x, n_hidden=1):
    h = x
    for i in range(n_hidden):
        h = F.relu(F.linear(h, sd[f"fc{i}.weight"], sd[f"fc{i}.bias"]))
    return h


@pytest.mark.parametrize("kind,K,dims", [("goac", 2, (1, 1, 16)), ("ptrain", 10, (5, 2, 24))])
def test_critic_eval_and_input_gradient_at_depth_1(kind, K, dims):
    """qfs[0](obs, act) and its input gradient against torch autograd on a
    float64 CPU copy of the weights."""
    Do, Da, H = dims
    tr = sl.trainer_for(_meta(kind, Do, Da, [H], K=K, q_init_w=0.3))
    qf = tr.qfs[0]
    assert [m for m, _ in qf.named_children()] == ["fc0", "last_fc"] and qf.fcs == [qf.fc0]
    rs = np.random.RandomState(3)
    N = 37
    obs = torch.tensor(rs.standard_normal((N, Do)), dtype=torch.float32, device="cuda:0",
                       requires_grad=True)
    act = torch.tensor(rs.uniform(-1, 1, (N, Da)), dtype=torch.float32, device="cuda:0",
                       requires_grad=True)
    from oac_amd.networks import critics_apply
    q = critics_apply([qf], obs, act)           # raw outputs (before any `positive` exp)
    w = torch.tensor(rs.standard_normal((N, K)), dtype=torch.float32, device="cuda:0")
    go, ga = torch.autograd.grad((q * w).sum(), (obs, act))
    sd = {k: v.detach().cpu().double() for k, v in qf.state_dict().items()}
    o64 = obs.detach().cpu().double().requires_grad_()
    a64 = act.detach().cpu().double().requires_grad_()
    qr = F.linear(_cpu_mlp(sd, torch.cat([o64, a64], 1)), sd["last_fc.weight"], sd["last_fc.bias"])
    gro, gra = torch.autograd.grad((qr * w.cpu().double()).sum(), (o64, a64))
    assert parity.rel_err(q.detach().cpu().numpy(), qr.detach().numpy()) < 1e-5
    assert parity.rel_err(go.cpu().numpy(), gro.numpy()) < 1e-5
    assert parity.rel_err(ga.cpu().numpy(), gra.numpy()) < 1e-5
    # the module's forward applies the reference's `positive` exp; predict runs on it
    out = qf(obs.detach(), act.detach())
    want = qr.detach().clone()
    if kind == "goac":
        want[:, 1] = torch.exp(want[:, 1])
    assert parity.rel_err(out.cpu().numpy(), want.numpy()) < 1e-5
    ub = tr.predict(obs.detach().cpu().numpy(), act.detach().cpu().numpy())
    assert torch.isfinite(ub[1] if isinstance(ub, tuple) else ub).all()


@pytest.mark.parametrize("N", [1, 37])
@pytest.mark.parametrize("dims", [(1, 1, 16), (5, 2, 24)])
def test_policy_eval_at_depth_1(N, dims):
    """The policy forward's 6-tuple (trainer/policies.py:260-316), deterministic
    and sampled with known eps, against a float64 CPU copy of the weights."""
    Do, Da, H = dims
    tr = sl.trainer_for(_meta("goac", Do, Da, [H], pi_init_w=0.05))
    pol = tr.policy
    assert [m for m, _ in pol.named_children()] == ["fc0", "last_fc", "last_fc_log_std"]
    assert pol.fcs == [pol.fc0]
    sd = {k: v.detach().cpu().double() for k, v in pol.state_dict().items()}
    obs = np.random.RandomState(4).standard_normal((N, Do)).astype(np.float32)
    h = _cpu_mlp(sd, torch.tensor(obs, dtype=torch.float64))
    mean_r = F.linear(h, sd["last_fc.weight"], sd["last_fc.bias"])
    ls_r = torch.clamp(F.linear(h, sd["last_fc_log_std.weight"], sd["last_fc_log_std.bias"]),
                       -20, 2)
    std_r = torch.exp(ls_r)
    rel = lambda got, ref: parity.rel_err(got.cpu().numpy(), ref.numpy())
    a, mean, log_std, lp, std, pre = pol(torch.tensor(obs), deterministic=True)
    assert a.shape == (N, Da)
    assert rel(mean, mean_r) < 1e-5 and rel(log_std, ls_r) < 1e-5 and rel(std, std_r) < 1e-5
    assert rel(a, torch.tanh(mean_r)) < 1e-5
    assert torch.equal(pre, mean) and lp.shape == a.shape and not lp.any()
    torch.manual_seed(5)
    eps = torch.randn(N, Da, device="cuda:0").cpu().double()
    torch.manual_seed(5)
    a, mean, log_std, lp, std, z = pol(torch.tensor(obs), return_log_prob=True)
    z_r = mean_r + std_r * eps
    a_r = torch.tanh(z_r)
    lp_r = (torch.distributions.Normal(mean_r, std_r).log_prob(z_r)
            - torch.log(1 - a_r * a_r + 1e-6)).sum(dim=1, keepdim=True)
    assert rel(z, z_r) < 1e-5 and rel(a, a_r) < 1e-5 and rel(mean, mean_r) < 1e-5
    assert lp.shape == (N, 1) and rel(lp, lp_r) < 1e-5
    # rollouts: one 1-D observation in, one [Da] action out
    act, info = pol.get_action(obs[0], deterministic=True)
    assert act.shape == (Da,) and info == {}
    assert parity.rel_err(act, torch.tanh(mean_r[0]).numpy()) < 1e-5
    from oac_amd.networks import MakeDeterministic
    act2, _ = MakeDeterministic(pol).get_action(obs[0])
    assert np.array_equal(act, act2)


# ---------------------------------------------------------------- snapshots
def _cpu(t):
    return torch.as_tensor(t).detach().cpu()


@pytest.mark.parametrize("name", ["goac_d1_counts", "ptrain_d1_counts"])
def test_own_snapshot_roundtrip_resumes_bitwise(name):
    meta, g = parity.load(name)

    def step(tr, s):
        r = np.random.RandomState(200 + s)
        b = batch_from(meta, r.randint(0, meta["n_replay"], meta["B"]))
        b["counts"] = (r.randint(0, 3, (meta["B"], 1)) * (r.uniform(0, 1, (meta["B"], 1)) < 0.5))
        tr.train_from_torch(b)

    a = sl.trainer_for(meta)
    for s in range(3):
        step(a, s)
    buf = io.BytesIO()
    torch.save(a.get_snapshot(), buf)
    buf.seek(0)
    ss = torch.load(buf, weights_only=True)
    assert list(ss["policy_state_dict"]) == sl.orders(1)[0]
    assert list(ss["qfs_state_dicts"][0]) == sl.orders(1)[1]
    assert sorted(ss["policy_optim_state_dict"]["state"]) == [0, 1, 2, 3]
    b = sl.trainer_for(meta)
    b.restore_from_snapshot(ss)
    for s in range(3, 5):
        step(a, s)
        step(b, s)
    torch.cuda.synchronize()
    for arena in ("params", "targets", "adam_m", "adam_v"):
        np.testing.assert_array_equal(getattr(a, arena).cpu().numpy(),
                                      getattr(b, arena).cpu().numpy())


def test_reference_depth_1_checkpoint_restores_and_resumes():
    """A checkpoint the reference's GaussianTrainer wrote at --num_layers 1
    restores with the same keys, tensors and Adam state layout, and the next
    step matches the reference's (1e-5 on every tensor: no wider than the gate)."""
    fx = torch.load(os.path.join(HERE, "golden", "goac_d1_snapshot.pt"), weights_only=True)
    meta = dict(fx["meta"], counts=True, soft=None)
    assert meta["hidden"] == [16] and meta["kind"] == "goac"
    tr = sl.trainer_for(meta)
    ref = fx["snapshot"]
    tr.restore_from_snapshot(ref)
    ours = tr.get_snapshot()
    assert set(ours) == set(ref)
    for key in ("policy_state_dict", "target_policy_state_dict"):
        assert list(ours[key]) == list(ref[key])
        for k, v in ref[key].items():
            torch.testing.assert_close(_cpu(ours[key][k]), v, rtol=0, atol=0)
    for key in ("qfs_state_dicts", "target_qfs_state_dicts"):
        assert list(ours[key][0]) == list(ref[key][0])
        for k, v in ref[key][0].items():
            torch.testing.assert_close(_cpu(ours[key][0][k]), v, rtol=0, atol=0)
    for so_, sr in ((ours["policy_optim_state_dict"], ref["policy_optim_state_dict"]),
                    (ours["target_policy_opt_state_dict"], ref["target_policy_opt_state_dict"]),
                    (ours["qfs_optims_state_dicts"][0], ref["qfs_optims_state_dicts"][0])):
        assert sorted(so_["state"]) == sorted(sr["state"])
        for i in sr["state"]:
            assert int(so_["state"][i]["step"]) == int(sr["state"][i]["step"])
            for f in ("exp_avg", "exp_avg_sq"):
                torch.testing.assert_close(
                    _cpu(so_["state"][i][f]).reshape(sr["state"][i][f].shape), sr["state"][i][f],
                    rtol=0, atol=0)
    s3 = fx["step3"]
    b = batch_from(meta, s3["idx"].numpy())
    b["counts"] = s3["counts"].numpy()
    tr.train_from_torch(b)
    torch.cuda.synchronize()
    mods = dict(policy=tr.policy, target_policy=tr.target_policy, qf=tr.q, tf=tr.q_target)
    worst = {}
    for grp, mod in mods.items():
        sd = mod.state_dict()
        for k, v in s3["post"][grp].items():
            worst[f"{grp}/{k}"] = parity.rel_err(_cpu(sd[k]).numpy(), v.numpy())
    print(sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    assert max(worst.values()) < 1e-5, worst


# -------------------------------------------------------------- entry paths
def _state(tr):
    torch.cuda.synchronize()
    return torch.cat([tr.params, tr.targets, tr.adam_m, tr.adam_v]).cpu().numpy()


@pytest.mark.parametrize("kind,K", [("goac", 2), ("ptrain", 10)])
def test_entry_paths_agree_bitwise(kind, K):
    """The same minibatches through the batch given as arrays, the drop-in
    random_batch + train call (host indices), the device index path and the
    device ring (train_from_ring)."""
    from oac_amd import DeviceIndexStream, ReplayBuffer
    Do, Da, B, N, steps = 1, 1, 32, 400, 5
    meta = _meta(kind, Do, Da, [16], K=K, counts=False, lr=1e-3)
    data = synthetic_transitions(N, Do, Da, seed=1)

    def replay():
        rb = ReplayBuffer(N, Space(Do), Space(Da), device="cuda:0")
        rb.add_paths([dict(observations=data["observations"], actions=data["actions"],
                           rewards=data["rewards"], next_observations=data["next_observations"],
                           terminals=data["terminals"])])
        return rb

    states, drawn = {}, []
    for path in ("dropin", "device_idx"):
        tr, rb = sl.trainer_for(meta), replay()
        tr._no_dropin = path != "dropin"
        np.random.seed(3)
        for _ in range(steps):
            batch = rb.random_batch(B)
            if path == "dropin":
                drawn.append(np.array(batch.host_indices))
            batch["buffer"] = rb
            tr.train(batch)
        states[path] = _state(tr)
    tr = sl.trainer_for(meta)
    for idx in drawn:
        tr.train_from_torch({k: v[idx] for k, v in data.items()})
    states["given"] = _state(tr)
    assert np.isfinite(states["given"]).all()
    np.testing.assert_array_equal(states["given"], states["dropin"])
    np.testing.assert_array_equal(states["given"], states["device_idx"])
    # the device ring draws its own indices: replay them through the given-batch path
    tr, rb = sl.trainer_for(meta), replay()
    st = DeviceIndexStream(rb, B, chunk=8, seed=4)
    st.before_step(4)
    torch.cuda.synchronize()
    ring = st.ring.view(st.slots, B)[:4].cpu().numpy().astype(np.int64)
    tr.train_from_ring(rb._storage, st.ring, st.slots, B, n_steps=4)
    tr2 = sl.trainer_for(meta)
    for idx in ring:
        tr2.train_from_torch({k: v[idx] for k, v in data.items()})
    np.testing.assert_array_equal(_state(tr), _state(tr2))


# ------------------------------------------------------------------ depths
def test_mixed_and_unsupported_depths_raise():
    from oac_amd import DDPGTrainer, GaussianTrainer, ParticleTrainerOAC, SACTrainer
    m1, m2 = _meta("goac", 5, 2, [24]), _meta("goac", 5, 2, [24, 24])
    p1, p2 = sl.params_of(m1), sl.params_of(m2)
    mixed = dict(p1, qf1=p2["qf1"], target_qf1=p2["target_qf1"])
    with pytest.raises(ValueError, match="same depth"):
        sl.trainer_for(m1, params=mixed)
    with pytest.raises(ValueError, match="same depth"):
        sl.trainer_for(m1, params=dict(p2, qf1=p1["qf1"], target_qf1=p1["target_qf1"]))
    m3 = _meta("goac", 5, 2, [24, 24, 24])
    with pytest.raises(ValueError, match="3 hidden layers"):
        sl.trainer_for(m3)
    # the other trainers keep their two layers, and say who takes one
    pol = lambda **k: StateDictModule(p1["policy"])
    q1 = dict(p1["qf1"])
    q1["last_fc.weight"], q1["last_fc.bias"] = q1["last_fc.weight"][:1], q1["last_fc.bias"][:1]
    qf = lambda **k: StateDictModule(q1)
    for make in (lambda: SACTrainer(pol, qf, action_space=Space(2)),
                 lambda: DDPGTrainer(pol, qf, action_space=Space(2)),
                 lambda: ParticleTrainerOAC(pol, lambda **k: StateDictModule(p1["qf1"]),
                                            n_estimators=2, action_space=Space(2),
                                            share_layers=True, deterministic=False)):
        with pytest.raises(ValueError, match="GaussianTrainer and ParticleTrainer"):
            make()
    assert GaussianTrainer is not None
