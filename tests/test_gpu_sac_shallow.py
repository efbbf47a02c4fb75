"""One-hidden-layer SAC / OAC on the GPU (``oac_amd.ShallowSACTrainer``,
OAC_KIND_SAC_SHALLOW, csrc/sac_shallow_plan.hip): the step against the
reference's own runs (tests/golden/sac_d1_*.npz) and against the fp32 CPU
oracle from the trainer's own state, its launch count, the call paths, the
device noise, checkpoints and what the class and the C ABI refuse.

No allowance anywhere: every tensor is compared whole (parity.rel_err /
parity.compare, no Adam sign band, no ReLU-boundary rows); a gate is 1e-5 or,
where larger, 3x the fp32 oracle's own distance from the float64 oracle on the
same inputs (parity.gate's rule) -- never a figure of the GPU's."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import parity
import sac_shallow_lib as ssl
import test_oracle_golden as tog
from fixtures_lib import sac_params, synthetic_transitions
from gpu_helpers import Space, StateDictModule, batch_from, producers, sac_trainer_for
from oracle.philox_oracle import philox_normal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LAUNCHES = 7          # the chain DESIGN.md section 15 states (batch and eps given: no gather launch)


# ----------------------------------------------------------- golden parity
@pytest.mark.parametrize("name", ssl.STEP_FIXTURES)
def test_step_matches_reference_golden(name):
    """Every gradient, post-step parameter, target, Adam moment and the
    statistics (keys in the reference's order), at every step, under
    parity.gate of the reference recording."""
    meta, g = parity.load(name)
    tr = ssl.trainer_for(meta)
    assert tr.n_hidden == 1
    errs = ssl.record_errors(meta, g, ssl.trainer_record(meta, g, tr))
    noise = ssl.oracle_noise(meta, g)
    bad = tog.gated(errs, noise)
    print(name, "worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


# ------------------------------------------------- oracle from own state
# (the helpers live in sac_shallow_lib: tests/test_gpu_shallow_wide.py runs them too)
_oracle_from = ssl.oracle_from
_step_against_oracle = ssl.step_against_oracle


@pytest.mark.parametrize("name", ssl.STEP_FIXTURES)
def test_every_step_matches_the_oracle_from_the_trainers_own_state(name):
    meta, g = parity.load(name)
    tr = ssl.trainer_for(meta)
    bad = {}
    for s in range(meta["steps"]):
        b = _step_against_oracle(tr, meta, batch_from(meta, g[f"s{s}/idx"]), g[f"s{s}/eps1"],
                                 g[f"s{s}/eps2"], f"{name} step {s}")
        bad.update({f"s{s}/{k}": v for k, v in b.items()})
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:10]


def _meta(Do, Da, H, **kw):
    m = dict(obs_dim=Do, act_dim=Da, hidden=[H], seed=3, pi_init_w=0.2, q_init_w=0.1, discount=0.99,
             reward_scale=1.0, lr=1e-3, tau=5e-3, auto_alpha=True, log_alpha0=0.0,
             target_update_period=1)
    m.update(kw)
    return m


def _batch(Do, Da, B, seed):
    data = synthetic_transitions(max(4 * B, 64), Do, Da, seed=seed)
    idx = np.random.RandomState(seed).randint(0, len(data["rewards"]), B)
    rs = np.random.RandomState(seed + 1)
    eps = [rs.standard_normal((B, Da)).astype(np.float32) for _ in range(2)]
    return {k: v[idx] for k, v in data.items()}, eps[0], eps[1]


# (Do, Da, H, B): B = 1; a ragged shape with more than one row block; B = 600:
# the small-batch kernels with split-K slabs and the two unfused Adam launches
@pytest.mark.parametrize("Do,Da,H,B", [(1, 1, 16, 1), (5, 2, 24, 1), (7, 5, 48, 300), (5, 2, 24, 600),
                                       (1, 1, 8, 600)])
def test_two_steps_against_the_oracle_at_other_batch_sizes(Do, Da, H, B):
    from oac_amd import _lib
    meta = _meta(Do, Da, H)
    tr = ssl.trainer_for(meta)
    bad = {}
    for s in range(2):
        batch, e1, e2 = _batch(Do, Da, B, 6 + s)
        b = _step_against_oracle(tr, meta, batch, e1, e2, f"({Do},{Da},{H}) B={B} step {s}")
        bad.update({f"s{s}/{k}": v for k, v in b.items()})
    fused = bool(_lib.lib().oac_sac_trace(tr._last_plan.handle, 0) & _lib.TRACE["fused"])
    n = _lib.lib().oac_sac_launch_count(tr._last_plan.handle)
    print(f"B={B}: fused {fused}, {n} launches")
    assert fused == (B < 512) and n == (LAUNCHES if fused else LAUNCHES + 2)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:10]


# ---------------------------------------------------------- launch count
def _launches(tr):
    from oac_amd import _lib
    return _lib.lib().oac_sac_launch_count(tr._last_plan.handle)


def test_launch_count():
    """Batch and eps given: the depth-1 step takes the 7 launches DESIGN.md
    states, strictly fewer than the two-layer SACTrainer at [16, 16] in the same
    test; with device eps each has one gather launch more."""
    n = {}
    for hidden in ([16], [16, 16]):
        meta = _meta(1, 1, 16, hidden=hidden)
        tr = ssl.trainer_for(meta) if len(hidden) == 1 else sac_trainer_for(meta)
        batch, e1, e2 = _batch(1, 1, 32, 6)
        tr.train_from_torch(batch, eps1=e1, eps2=e2)
        torch.cuda.synchronize()
        given = _launches(tr)
        tr.train_from_torch(batch)
        torch.cuda.synchronize()
        n[len(hidden)] = (given, _launches(tr))
    print("launches (eps given, device eps):", n)
    assert n[1] == (LAUNCHES, LAUNCHES + 1)
    assert n[1][0] < n[2][0] and n[1][1] < n[2][1]


# -------------------------------------------------------------- call paths
def _state(tr):
    torch.cuda.synchronize()
    return torch.cat([tr.params, tr.targets, tr.adam_m, tr.adam_v, tr.alpha_state]).cpu().numpy()


def test_entry_paths_agree_bitwise():
    """The same minibatches (device Philox eps: the same counters) through the
    batch given as arrays, the drop-in random_batch + train call (host indices
    read by the layer-0 launch), the device index path and the device ring."""
    from oac_amd import DeviceIndexStream, ReplayBuffer, _lib
    Do, Da, B, N, steps = 1, 1, 32, 400, 5
    meta = _meta(Do, Da, 16)
    data = synthetic_transitions(N, Do, Da, seed=1)

    def replay():
        rb = ReplayBuffer(N, Space(Do), Space(Da), device="cuda:0")
        rb.add_paths([dict(observations=data["observations"], actions=data["actions"],
                           rewards=data["rewards"], next_observations=data["next_observations"],
                           terminals=data["terminals"])])
        return rb

    states, drawn = {}, []
    for path in ("dropin", "device_idx"):
        tr, rb = ssl.trainer_for(meta), replay()
        tr._no_dropin = path != "dropin"
        np.random.seed(3)
        for _ in range(steps):
            batch = rb.random_batch(B)
            if path == "dropin":
                drawn.append(np.array(batch.host_indices))
            batch["buffer"] = rb
            tr.train(batch)
        states[path] = _state(tr)
        bits = _lib.lib().oac_sac_trace(tr._last_plan.handle, 0)
        assert bool(bits & _lib.TRACE["direct"]) == (path == "dropin")
        assert _launches(tr) == (LAUNCHES if path == "dropin" else LAUNCHES + 1)
    tr = ssl.trainer_for(meta)
    for idx in drawn:
        tr.train_from_torch({k: v[idx] for k, v in data.items()})
    states["given"] = _state(tr)
    assert np.isfinite(states["given"]).all()
    np.testing.assert_array_equal(states["given"], states["dropin"])
    np.testing.assert_array_equal(states["given"], states["device_idx"])
    # the device ring draws its own indices: replay them through the given-batch path
    tr, rb = ssl.trainer_for(meta), replay()
    st = DeviceIndexStream(rb, B, chunk=8, seed=4)
    st.before_step(4)
    torch.cuda.synchronize()
    ring = st.ring.view(st.slots, B)[:4].cpu().numpy().astype(np.int64)
    tr.train_from_ring(rb._storage, st.ring, st.slots, B, n_steps=4)
    tr2 = ssl.trainer_for(meta)
    for idx in ring:
        tr2.train_from_torch({k: v[idx] for k, v in data.items()})
    np.testing.assert_array_equal(_state(tr), _state(tr2))


@pytest.mark.parametrize("B", [37, 600])
def test_two_runs_from_the_same_state_are_bitwise_equal(B):
    meta = _meta(5, 2, 24)
    outs = []
    for _ in range(2):
        tr = ssl.trainer_for(meta)
        for s in range(3):
            batch, e1, e2 = _batch(5, 2, B, 6 + s)
            tr.train_from_torch(batch, eps1=e1, eps2=e2)
        tr.train_from_torch(batch)           # device eps too
        outs.append(np.concatenate([_state(tr), tr.grads.cpu().numpy()]))
    np.testing.assert_array_equal(outs[0], outs[1])


# ------------------------------------------------------------ device noise
@pytest.mark.parametrize("path", ["given", "dropin"])
def test_device_eps_follow_the_philox_contract(path):
    """OAC_STEP_DEVICE_EPS draws of two consecutive steps against
    oracle/philox_oracle.py: eps_s[e] = philox_normal(seed, batch_counter, s,
    e), s = 1, 2 -- the two-layer SAC step's contract, from the gather launch
    (batch given) and from the layer-0 launch's side blocks (drop-in).
    Allowance 4 x the restatement's own float32 rounding, as
    tests/test_gpu_noise.py."""
    from oac_amd import ReplayBuffer, _lib
    Do, Da, B = 7, 5, 37
    tr = ssl.trainer_for(_meta(Do, Da, 48), seed=7)
    tr.step_state[1] = 2 ** 32 + 3   # (the counter's high word)
    data = synthetic_transitions(500, Do, Da, seed=1)
    rb = ReplayBuffer(500, Space(Do), Space(Da), device="cuda:0")
    rb.add_paths([dict(observations=data["observations"], actions=data["actions"],
                       rewards=data["rewards"], next_observations=data["next_observations"],
                       terminals=data["terminals"])])
    np.random.seed(5)
    misses = []
    for k in range(2):
        c0 = int(tr.step_state[1].item())
        if path == "given":
            plan = tr._plan(B)
            for s in (1, 2):
                plan.views[f"eps{s}"].fill_(float("nan"))
            tr.train_from_torch({kk: v[:B] for kk, v in data.items()})
        else:
            batch = rb.random_batch(B)
            plan = tr._dropin_plan(batch)
            for s in (1, 2):
                plan.views[f"eps{s}"].fill_(float("nan"))
            batch["buffer"] = rb
            tr.train(batch)
        torch.cuda.synchronize()
        assert plan is tr._last_plan and int(tr.step_state[1].item()) == c0 + 1
        bits = _lib.lib().oac_sac_trace(plan.handle, 1)
        assert bool(bits & _lib.TRACE["direct"]) == (path == "dropin")
        idx = np.arange(B * Da)
        for s in (1, 2):
            got = plan.views[f"eps{s}"].cpu().numpy().astype(np.float64).reshape(-1)
            assert not np.isnan(got).any()
            ref = philox_normal(tr.seed, c0, s, idx, np.float64)
            noise = np.abs(philox_normal(tr.seed, c0, s, idx, np.float32).astype(np.float64) - ref).max()
            d = np.abs(got - ref).max()
            print(f"{path} step {k} eps{s}: device-oracle {d:.3e}, allowance {4 * noise:.3e}")
            if not d <= 4 * noise:
                misses.append((path, k, s, d, noise))
    assert not misses, misses


# ---------------------------------------------------------------- snapshots
def _cpu(t):
    return torch.as_tensor(t).detach().cpu()


def test_own_snapshot_roundtrip_resumes_bitwise():
    meta, g = parity.load("sac_d1_riverswim")

    def step(tr, s):
        r = np.random.RandomState(200 + s)
        b = batch_from(meta, r.randint(0, meta["n_replay"], meta["B"]))
        e = [r.standard_normal((meta["B"], meta["act_dim"])).astype(np.float32) for _ in range(2)]
        tr.train_from_torch(b, eps1=e[0], eps2=e[1])

    a = ssl.trainer_for(meta)
    for s in range(3):
        step(a, s)
    buf = io.BytesIO()
    torch.save(a.get_snapshot(), buf)
    buf.seek(0)
    ss = torch.load(buf, weights_only=True)
    from shallow_lib import orders
    assert list(ss["policy_state_dict"]) == orders(1)[0]
    assert list(ss["qf1_state_dict"]) == orders(1)[1] == list(ss["target_qf2_state_dict"])
    assert sorted(ss["policy_optim_state_dict"]["state"]) == list(range(6))
    assert sorted(ss["qf2_optim_state_dict"]["state"]) == list(range(4))
    b = ssl.trainer_for(meta)
    b.restore_from_snapshot(ss)
    for s in range(3, 5):
        step(a, s)
        step(b, s)
    np.testing.assert_array_equal(_state(a), _state(b))


def test_reference_depth_1_checkpoint_restores_and_resumes():
    """A checkpoint the reference's SACTrainer wrote at --num_layers 1 restores
    with the same keys, tensors and Adam state layout, and the next step
    matches the reference's (1e-5 on every tensor: no wider than the gate)."""
    fx = torch.load(os.path.join(HERE, "golden", "sac_d1_snapshot.pt"), weights_only=True)
    m = fx["meta"]
    assert m["hidden"] == [16]
    meta = _meta(m["obs_dim"], m["act_dim"], 16, seed=m["seed"], lr=m["lr"], tau=m["tau"],
                 n_replay=m["n_replay"])
    tr = ssl.trainer_for(meta)
    ref = fx["snapshot"]
    tr.restore_from_snapshot(ref)
    ours = tr.get_snapshot()
    assert set(ours) == set(ref)
    for key in ("policy_state_dict", "qf1_state_dict", "qf2_state_dict", "target_qf1_state_dict",
                "target_qf2_state_dict"):
        assert list(ours[key]) == list(ref[key])
        for k, v in ref[key].items():
            torch.testing.assert_close(_cpu(ours[key][k]), v, rtol=0, atol=0)
    for key in ("policy_optim_state_dict", "qf1_optim_state_dict", "qf2_optim_state_dict",
                "alpha_optim_state_dict"):
        so_, sr = ours[key], ref[key]
        assert sorted(so_["state"]) == sorted(sr["state"])
        for i in sr["state"]:
            assert int(so_["state"][i]["step"]) == int(sr["state"][i]["step"])
            for f in ("exp_avg", "exp_avg_sq"):
                torch.testing.assert_close(_cpu(so_["state"][i][f]).reshape(sr["state"][i][f].shape),
                                           sr["state"][i][f], rtol=0, atol=0)
    torch.testing.assert_close(_cpu(ours["log_alpha"]).reshape(-1), _cpu(ref["log_alpha"]).reshape(-1),
                               rtol=0, atol=0)
    s3 = fx["step3"]
    tr.train_from_torch(batch_from(meta, s3["idx"].numpy()), eps1=s3["eps1"].numpy(),
                        eps2=s3["eps2"].numpy())
    torch.cuda.synchronize()
    worst = {}
    for grp in ssl.GROUPS + ssl.TARGETS:
        sd = getattr(tr, grp).state_dict()
        for k, v in s3["post"][grp].items():
            worst[f"{grp}/{k}"] = parity.rel_err(_cpu(sd[k]).numpy(), v.numpy())
    worst["log_alpha"] = parity.rel_err(_cpu(tr.log_alpha).numpy(), s3["log_alpha"].numpy())
    print(sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    assert max(worst.values()) < 1e-5, worst


# ------------------------------------------------------------------ refusals
def test_what_the_class_and_the_abi_refuse():
    from oac_amd import DDPGTrainer, ParticleTrainerOAC, SACTrainer, ShallowSACTrainer, _lib
    p1 = sac_params(5, 2, [24], 3, pi_init_w=0.2, q_init_w=0.1)
    p2 = sac_params(5, 2, [24, 24], 3, pi_init_w=0.2, q_init_w=0.1)
    mk = lambda cls, p, **kw: cls(*producers(p), action_space=Space(2), **kw)
    # two-layer producers: pointed at SACTrainer; mixed depths; another depth
    with pytest.raises(ValueError, match="SACTrainer"):
        mk(ShallowSACTrainer, p2)
    with pytest.raises(ValueError, match="same depth"):
        mk(ShallowSACTrainer, dict(p1, qf1=p2["qf1"], qf2=p2["qf2"], target_qf1=p2["target_qf1"],
                                   target_qf2=p2["target_qf2"]))
    with pytest.raises(ValueError, match="3 hidden layers"):
        mk(ShallowSACTrainer, sac_params(5, 2, [24, 24, 24], 3))
    with pytest.raises(ValueError, match="multiple of 4"):
        mk(ShallowSACTrainer, sac_params(5, 2, [18], 3))
    with pytest.raises(NotImplementedError, match="use_graph"):
        mk(ShallowSACTrainer, p1, use_graph=True)
    # the others keep their two layers, and SACTrainer's message names the new class
    with pytest.raises(ValueError, match="GaussianTrainer and ParticleTrainer.*ShallowSACTrainer"):
        mk(SACTrainer, p1)
    with pytest.raises(ValueError, match="GaussianTrainer and ParticleTrainer"):
        mk(DDPGTrainer, p1)
    with pytest.raises(ValueError, match="GaussianTrainer and ParticleTrainer"):
        ParticleTrainerOAC(lambda **k: StateDictModule(p1["policy"]),
                           lambda **k: StateDictModule(sac_params(5, 2, [24], 3, q_out=2)["qf1"]),
                           n_estimators=2, action_space=Space(2), share_layers=True,
                           deterministic=False)
    # a batch that selects the large-batch kernel set: refused at plan creation, by name
    tr = mk(ShallowSACTrainer, p1)
    assert tr._kind == _lib.OAC_KIND_SAC_SHALLOW == 5 and tr.n_hidden == 1
    assert [m for m, _ in tr.policy.named_children()] == ["fc0", "last_fc", "last_fc_log_std"]
    assert [m for m, _ in tr.qf1.named_children()] == ["fc0", "last_fc"]
    assert len(tr.networks) == 5
    batch, e1, e2 = _batch(5, 2, 1024, 6)
    with pytest.raises(RuntimeError, match="SAC_SHALLOW.*large-batch"):
        tr.train_from_torch(batch, eps1=e1, eps2=e2)
    # the C ABI on a live handle: no graph, no data-parallel entry points
    batch, e1, e2 = _batch(5, 2, 32, 6)
    tr.train_from_torch(batch, eps1=e1, eps2=e2)
    h = tr._last_plan.handle
    L = _lib.lib()
    s = _lib.stream_ptr(tr.stream)
    before = _state(tr)
    assert L.oac_sac_step(h, _lib.OAC_STEP_USE_GRAPH, s) != 0
    assert b"OAC_STEP_USE_GRAPH" in L.oac_last_error() and b"SAC_SHALLOW" in L.oac_last_error()
    assert L.oac_sac_step_phase(h, 0, 0, s) != 0 and b"oac_sac_step_phase" in L.oac_last_error()
    assert L.oac_sac_set_allreduce(h, None, None, 0) != 0 and b"SAC_SHALLOW" in L.oac_last_error()
    np.testing.assert_array_equal(before, _state(tr))   # nothing ran
    # exploration on this trainer: no K-head form
    e = tr._expl_handle(1)
    assert L.oac_expl_set_ub_index(e.handle, 0) != 0 and b"K-head" in L.oac_last_error()


def test_policy_and_critic_evaluation_at_depth_1():
    """policy.get_action / MakeDeterministic / trainer.predict on the trainer's
    arena networks (csrc/mlp_eval.hip at offsets[2] = -1), stochastic head
    included, against a float64 CPU copy of the weights."""
    import torch.nn.functional as F
    from oac_amd.networks import MakeDeterministic
    Do, Da, H, N = 5, 2, 24, 37
    tr = ssl.trainer_for(_meta(Do, Da, H))
    pol = tr.policy
    sd = {k: v.detach().cpu().double() for k, v in pol.state_dict().items()}
    obs = np.random.RandomState(4).standard_normal((N, Do)).astype(np.float32)
    h = F.relu(F.linear(torch.tensor(obs, dtype=torch.float64), sd["fc0.weight"], sd["fc0.bias"]))
    mean_r = F.linear(h, sd["last_fc.weight"], sd["last_fc.bias"])
    std_r = torch.exp(torch.clamp(F.linear(h, sd["last_fc_log_std.weight"], sd["last_fc_log_std.bias"]),
                                  -20, 2))
    rel = lambda got, ref: parity.rel_err(got.cpu().numpy(), ref.numpy())
    torch.manual_seed(5)
    eps = torch.randn(N, Da, device="cuda:0").cpu().double()
    torch.manual_seed(5)
    a, mean, log_std, lp, std, z = pol(torch.tensor(obs), return_log_prob=True)
    z_r = mean_r + std_r * eps
    a_r = torch.tanh(z_r)
    lp_r = (torch.distributions.Normal(mean_r, std_r).log_prob(z_r)
            - torch.log(1 - a_r * a_r + 1e-6)).sum(dim=1, keepdim=True)
    assert rel(mean, mean_r) < 1e-5 and rel(std, std_r) < 1e-5 and rel(z, z_r) < 1e-5
    assert rel(a, a_r) < 1e-5 and lp.shape == (N, 1) and rel(lp, lp_r) < 1e-5
    act, info = pol.get_action(obs[0], deterministic=True)
    assert act.shape == (Da,) and info == {}
    assert parity.rel_err(act, torch.tanh(mean_r[0]).numpy()) < 1e-5
    act2, _ = MakeDeterministic(pol).get_action(obs[0])
    assert np.array_equal(act, act2)
    # predict: Q_UB = (Q1 + Q2) / 2 + beta |Q1 - Q2| / 2 of the twin one-layer critics
    acts = np.random.RandomState(5).uniform(-1, 1, (N, Da)).astype(np.float32)
    x = torch.tensor(np.concatenate([obs, acts], 1), dtype=torch.float64)
    qs = []
    for qf in tr.qfs:
        q = {k: v.detach().cpu().double() for k, v in qf.state_dict().items()}
        qs.append(F.linear(F.relu(F.linear(x, q["fc0.weight"], q["fc0.bias"])), q["last_fc.weight"],
                           q["last_fc.bias"]))
    want = (qs[0] + qs[1]) / 2 + 4.66 * torch.abs(qs[0] - qs[1]) / 2
    ub = tr.predict(obs, acts, beta_UB=4.66)
    assert ub.shape == (N, 1) and rel(ub, want) < 1e-5
