"""share_layers=False (separate critics, each with its own optimizer) for the
g-oac GaussianTrainer and the p-oac ParticleTrainer on the GPU: the stacked
critic step (csrc/det_plan.hip, ``unshared``) against the reference's own
unshared runs (tests/golden/*_us_*.npz) and the CPU oracle
(tests/unshared_oracle.py), the reference's objects and snapshots, the entry
paths, the configurations that must raise, and the shared-layer step through
the kernels this feature changed."""
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity
import shallow_lib as sl
import test_oracle_golden as tog
import unshared_oracle as uo
from fixtures_lib import synthetic_transitions
from gpu_helpers import Space, batch_from, module_tensors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5


# (the helpers live in unshared_oracle: tests/test_gpu_shallow_wide.py runs them too)
oracle_from_gpu = uo.oracle_from_gpu
step_errors_against_oracle = uo.step_errors_against_oracle


# ----------------------------------------------------------- golden parity
@pytest.mark.parametrize("name", uo.FIXTURES)
def test_step_matches_reference_and_oracle_unshared(name):
    """Per fixture and per step, nothing left out: (teacher-forced) from the
    GPU trainer's own pre-step state every network's gradient, post-step
    parameters, Adam m / v and target within 1e-5 of the fp32 oracle's step;
    and along the trajectory the same quantities and the statistics (keys in
    the reference's order) against the reference's recording under the
    project's gate."""
    meta, g = parity.load(name)
    tr = uo.trainer_for(meta)
    assert tr.n_hidden == 1 and tr.unshared
    if meta.get("use_target_policy"):
        sl.load_tpn(tr, g)
    K = uo.n_critics(meta)
    assert len(tr.qfs) == len(tr.tfs) == len(tr.qf_optimizers) == K
    heads0 = {(m, k): getattr(tr, m).state_dict()[k].clone()
              for m in ("policy", "target_policy") for k in uo.POL_ORDER[-2:]}
    errs, forced = {}, {}
    for s in range(meta["steps"]):
        tr.end_epoch(s)
        b = batch_from(meta, g[f"s{s}/idx"])
        if meta["counts"]:
            b["counts"] = g[f"s{s}/counts"][:, None]
        orc = oracle_from_gpu(tr, meta, g)
        out = orc.step(b)
        tr.train_from_torch(b)
        for k, v in step_errors_against_oracle(tr, orc, out, meta).items():
            forced[f"s{s}/{k}"] = v
        groups = [("policy", tr.policy, uo.POL_ORDER, meta["lr"]),
                  ("target_policy", tr.target_policy, uo.POL_ORDER, meta["lr"])]
        groups += [(f"qf{k}", tr.qfs[k], uo.Q_ORDER, uo.critic_lr(meta, k)) for k in range(K)]
        for grp, mod, order, lr in groups:
            assert list(mod.state_dict()) == order
            gv = module_tensors(tr, mod, tr.grads)
            sd = mod.state_dict()
            for pn in order:
                key = f"s{s}/grad/{grp}/{pn}"
                errs[key] = parity.compare(g, key, gv[pn].cpu().numpy())
                key = f"s{s}/post/{grp}/{pn}"
                gk = f"s{s}/grad/{grp}/{pn}" if s == 0 else None
                errs[key], _ = parity.compare_post(g, key, gk, sd[pn].cpu().numpy(), lr)
        for k in range(K):
            mv = module_tensors(tr, tr.qfs[k], tr.adam_m)
            vv = module_tensors(tr, tr.qfs[k], tr.adam_v)
            for pn, t in tr.tfs[k].state_dict().items():
                errs[f"s{s}/post/tf{k}/{pn}"] = parity.compare(g, f"s{s}/post/tf{k}/{pn}",
                                                               t.cpu().numpy())
                errs[f"s{s}/adam_m/qf{k}/{pn}"] = parity.compare(g, f"s{s}/adam_m/qf{k}/{pn}",
                                                                 mv[pn].cpu().numpy())
                errs[f"s{s}/adam_v/qf{k}/{pn}"] = parity.compare(g, f"s{s}/adam_v/qf{k}/{pn}",
                                                                 vv[pn].cpu().numpy())
        keys = [k[len(f"s{s}/stat/"):] for k in g if k.startswith(f"s{s}/stat/")]
        assert list(tr.get_diagnostics().keys()) == keys
        for k, v in tr.get_diagnostics().items():
            errs[f"s{s}/stat/{k}"] = parity.stat_err(v, g, f"s{s}/stat/{k}")
    for (m, k), v in heads0.items():
        assert torch.equal(v, getattr(tr, m).state_dict()[k]), (m, k)
    print(name, "teacher-forced worst", sorted(forced.items(), key=lambda kv: -kv[1])[:3])
    print(name, "trajectory worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    bad = {k: v for k, v in forced.items() if v > TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:10]
    noise = uo.oracle_errors(meta, g, torch.float64)
    assert set(noise) <= set(errs)   # (errs also holds the integer out-of-order counts)
    bad = tog.gated(errs, noise)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]
    # Adam state as torch keeps it: none for a frozen last bias
    for k, opt in enumerate(tr.qf_optimizers):
        frozen = not meta["train_bias"] and (meta["kind"] == "ptrain" or k == 1)
        assert sorted(opt.state_dict()["state"]) == ([0, 1, 2] if frozen else [0, 1, 2, 3])
        assert opt.param_groups[0]["lr"] == uo.critic_lr(meta, k)


# ------------------------------------------------- one step against the oracle
def _meta(kind, Do, Da, H, K=2, **kw):
    m = dict(kind=kind, obs_dim=Do, act_dim=Da, hidden=[H], K=K, seed=3, q_min=0.0, q_max=50.0,
             pi_init_w=0.2, q_init_w=0.1, discount=0.99, delta=0.95, lr=3e-4, std_lr=1e-4,
             tau=5e-3, counts=True, n_replay=400)
    m.update(kw)
    return m


def _batch(Do, Da, B, seed):
    data = synthetic_transitions(max(4 * B, 64), Do, Da, seed=seed)
    idx = np.random.RandomState(seed).randint(0, len(data["rewards"]), B)
    b = {k: v[idx] for k, v in data.items()}
    b["counts"] = np.random.RandomState(seed + 1).randint(0, 2, (B, 1)).astype(np.float64)
    return b


def _one_step_against_oracle(meta, B, **kw):
    """One step from identical state: every gradient, post-step parameter,
    Adam moment and target within 1e-5 (norm-relative) of the fp32 oracle's."""
    tr = uo.trainer_for(meta, **kw)
    if meta["kind"] == "ptrain":
        meta = dict(meta, delta_index=tr.delta_index)
    b = _batch(meta["obs_dim"], meta["act_dim"], B, 6)
    if not meta["counts"]:
        b.pop("counts")
    orc = oracle_from_gpu(tr, meta)
    out = orc.step(b)
    tr.train_from_torch(b)
    worst = step_errors_against_oracle(tr, orc, out, meta)
    print(meta["kind"], meta["hidden"], meta["K"], B, sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    bad = {k: v for k, v in worst.items() if v > TOL}
    assert not bad, bad
    return tr, out


def _launches(tr):
    from oac_amd import _lib
    return _lib.lib().oac_sac_launch_count(tr._last_plan.handle)


# B = 1100: the large-batch kernel set, split-K slabs reduced before the critic
# block's optimizer launch; B = 600: the small-batch kernels with slabs
@pytest.mark.parametrize("kind,K,B", [("goac", 2, 1100), ("ptrain", 5, 1100), ("goac", 2, 600),
                                      ("ptrain", 3, 600)])
def test_one_step_with_split_k_slabs(kind, K, B):
    tr, _ = _one_step_against_oracle(_meta(kind, 5, 2, 24, K=K), B)
    assert _launches(tr) > 9   # (the slab reduction and the unfused policy Adam)


@pytest.mark.parametrize("kind,K,dims,B", [
    ("ptrain", 10, (3, 2, 32), 20),    # stacked width 320 > 256: row_heads' generic loop
    ("ptrain", 16, (1, 1, 16), 32),    # 16 critics: every lane of the MFMA's B operand
    ("ptrain", 2, (1, 1, 4), 1),       # one row, the narrowest block (8)
    ("goac", 2, (7, 5, 48), 300),      # several row blocks, Da > 4
    ("goac", 2, (1, 1, 16), 17)])      # a ragged last row block
def test_one_step_shapes(kind, K, dims, B):
    Do, Da, H = dims
    tr, _ = _one_step_against_oracle(_meta(kind, Do, Da, H, K=K), B)
    assert _launches(tr) == 9


@pytest.mark.parametrize("kind,K", [("goac", 2), ("ptrain", 5)])
def test_std_soft_update(kind, K):
    _one_step_against_oracle(_meta(kind, 5, 2, 24, K=K, counts=False, soft=0.3), 37)


def test_rescale_targets_around_mean():
    """A prior 0.5 wide under last-layer weights of +-0.5: target spreads
    above q_max - q_min, which the rescale shrinks around their mean."""
    meta = _meta("ptrain", 5, 2, 24, K=5, counts=False, rescale=True, q_max=0.5, q_init_w=0.5)
    tr, out = _one_step_against_oracle(meta, 37)
    plain = uo.make_oracle(dict(meta, rescale=False, delta_index=tr.delta_index)).step(
        {k: v for k, v in _batch(5, 2, 37, 6).items() if k != "counts"})
    assert not torch.equal(plain["y"], out["y"])   # (the option changed the targets)


@pytest.mark.parametrize("kind,K", [("goac", 2), ("ptrain", 10)])
def test_launch_count(kind, K):
    """Small batch, batch given: the shared depth-1 step's 8 launches and one
    more, which forms the block-diagonal last layer's gradient and steps the
    critic block (the count DESIGN.md records)."""
    meta = _meta(kind, 1, 1, 16, K=K)
    tr = uo.trainer_for(meta)
    tr.train_from_torch(_batch(1, 1, 32, 6))
    sh = sl.trainer_for(dict(meta))
    sh.train_from_torch(_batch(1, 1, 32, 6))
    torch.cuda.synchronize()
    assert (_launches(sh), _launches(tr)) == (8, 9)


# -------------------------------------------------- the reference's objects
def test_gaussian_objects_and_producer_calls():
    """gaussian_trainer.py:100-112: q, q_target, std, std_target built in that
    order with those keyword arguments; two optimizers at qf_lr / std_lr."""
    meta = _meta("goac", 1, 1, 16, train_bias=False)
    tr = uo.trainer_for(meta)
    mean, log_std = uo.critic_biases(meta)
    calls = tr.q_producer_calls[4:]
    assert [sorted(c) for c in calls] == [["bias"], ["bias"], ["bias", "positive", "train_bias"],
                                          ["bias", "positive", "train_bias"]]
    assert calls[0]["bias"] == calls[1]["bias"] == mean
    assert calls[2]["bias"] == calls[3]["bias"] == log_std
    assert calls[2]["positive"] is True and calls[2]["train_bias"] is False
    assert tr.qfs == [tr.q, tr.std] and tr.tfs == [tr.q_target, tr.std_target]
    assert tr.q_optimizer.param_groups[0]["lr"] == meta["lr"]
    assert tr.std_optimizer.param_groups[0]["lr"] == meta["std_lr"]
    for mod in tr.qfs + tr.tfs:
        sd = mod.state_dict()
        assert list(sd) == uo.Q_ORDER
        assert [tuple(v.shape) for v in sd.values()] == [(16, 2), (16,), (1, 16), (1,)]
    nets = tr.networks
    assert nets == [tr.policy, tr.q, tr.std, tr.q_target, tr.std_target, tr.target_policy]
    # each module is a view of its slice of the stacked critic block
    lay = tr.layout
    base = tr.params.data_ptr() + 4 * lay.q1_base
    assert tr.std.fc0.weight.data_ptr() == base + 4 * (lay.q_fc0_w + 16 * 2)
    assert tr.std.last_fc.bias.data_ptr() == base + 4 * (lay.q_last_b + 1)
    assert tr.std_target.last_fc.weight.data_ptr() == tr.targets.data_ptr() + 4 * (lay.q_last_w + 16)


def test_particle_objects_and_producer_calls():
    meta = _meta("ptrain", 1, 1, 16, K=10)
    tr = uo.trainer_for(meta)
    calls = tr.q_producer_calls[4:]
    init = uo.critic_biases(meta)
    assert len(calls) == 20 and all(sorted(c) == ["bias", "train_bias"] for c in calls)
    assert [c["bias"] for c in calls] == [b for b in init for _ in range(2)]
    assert len(tr.qfs) == len(tr.tfs) == len(tr.qf_optimizers) == 10
    assert tr.num_particles == tr.n_estimators == 10
    assert tr.networks == [tr.policy] + tr.qfs + tr.tfs + [tr.target_policy]
    for k, q in enumerate(tr.qfs):
        assert float(q.last_fc.bias) == np.float32(init[k])
        assert torch.equal(tr.tfs[k].fc0.weight, q.fc0.weight)   # (the target is a copy)


def _main_py_kwargs(alg, std_soft_update_prob=0.1):
    """main.py's trainer_kwargs for a riverswim / lqg recipe run without
    --share_layers (:198-233, 501-530, 547-555)."""
    kw = dict(discount=0.99, soft_target_tau=5e-3, target_update_period=1, policy_lr=3e-4,
              qf_lr=3e-4, use_automatic_entropy_tuning=True, std_soft_update=False,
              share_layers=False, mean_update=False, counts=False, global_opt=False,
              r_mellow_max=1.0, mellow_max=False, train_bias=True,
              rescale_targets_around_mean=False, use_target_policy=False,
              std_soft_update_prob=std_soft_update_prob)
    if alg == "g-oac":
        kw["std_lr"] = 3e-5
    return kw


@pytest.mark.parametrize("alg,H,K", [("g-oac", 16, 2), ("p-oac", 16, 10), ("p-oac", 8, 10)])
def test_recipe_constructions_are_accepted(alg, H, K):
    """g_oac.sh / w_oac.sh (riverswim, --num_layers 1 --layer_size 16) and
    reproduce.sh:6 (lqg, --layer_size 8 --n_estimators 10): main.py's trainer
    construction, with one-output producers, unchanged; then one step."""
    import oac_amd
    meta = _meta("goac" if alg == "g-oac" else "ptrain", 1, 1, H, K=K)
    pp, qp = uo.producers(uo.params_of(meta), meta["kind"])
    kw = dict(action_space=Space(1), delta=0.95, q_min=0.0, q_max=100.0, n_estimators=K,
              deterministic=True, policy_producer=pp, q_producer=qp, **_main_py_kwargs(alg))
    cls = oac_amd.GaussianTrainer if alg == "g-oac" else oac_amd.ParticleTrainer
    tr = cls(**kw)
    b = _batch(1, 1, 32, 6)
    b.pop("counts")
    tr.train(b)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.params).all() and len(tr.qfs) == K
    assert list(tr.qfs[0].state_dict()) == uo.Q_ORDER


# ----------------------------------------------------- diagnostics / predict
def _cpu_q(sd, x):
    h = F.relu(F.linear(x, sd["fc0.weight"], sd["fc0.bias"]))
    return F.linear(h, sd["last_fc.weight"], sd["last_fc.bias"])


@pytest.mark.parametrize("kind,K,dims", [("goac", 2, (1, 1, 16)), ("ptrain", 10, (5, 2, 24))])
def test_predict_and_obj_func_against_a_cpu_mlp(kind, K, dims):
    """predict / obj_func follow the reference's unshared branches
    (gaussian_trainer.py:161-175, 520-531; particle_trainer.py:157-173, 505-515)
    on float64 CPU copies of each critic's weights."""
    Do, Da, H = dims
    tr = uo.trainer_for(_meta(kind, Do, Da, H, K=K, q_init_w=0.3))
    rs = np.random.RandomState(3)
    obs = rs.standard_normal((37, Do)).astype(np.float32)
    act = rs.uniform(-1, 1, (37, Da)).astype(np.float32)
    x = torch.tensor(np.concatenate([obs, act], 1), dtype=torch.float64)
    outs = [_cpu_q({k: v.detach().cpu().double() for k, v in q.state_dict().items()}, x)
            for q in tr.qfs]
    rel = lambda got, ref: parity.rel_err(got.cpu().numpy(), ref.numpy())
    if kind == "goac":
        qs, stds = outs[0], torch.exp(outs[1])
        (gq, gs), ub = tr.predict(obs, act)
        assert gq.shape == gs.shape == ub.shape == (37, 1)
        assert rel(gq, qs) < TOL and rel(gs, stds) < TOL
        assert rel(ub, qs + tr.standard_bound * stds) < TOL
        assert rel(tr.predict(obs, act, std=False), qs + tr.standard_bound * stds) < TOL
        assert rel(tr.obj_func(obs, act), qs) < TOL
        assert rel(tr.obj_func(obs, act, upper_bound=True), qs + tr.standard_bound * stds) < TOL
    else:
        stack = torch.stack(outs, dim=0)                       # [K, N, 1]
        srt = torch.sort(stack, dim=0)[0]
        allp, ub = tr.predict(obs, act, all_particles=True)
        assert allp.shape == (K, 37, 1) and ub.shape == (37, 1)
        assert rel(allp, srt) < TOL and rel(ub, srt[tr.delta_index]) < TOL
        assert rel(tr.predict(obs, act), srt[tr.delta_index]) < TOL
        assert rel(tr.obj_func(obs, act), stack.mean(dim=0)) < TOL
        assert rel(tr.obj_func(obs, act, upper_bound=True), srt[tr.delta_index]) < TOL


# ---------------------------------------------------------------- snapshots
def _cpu(t):
    return torch.as_tensor(t).detach().cpu()


@pytest.mark.parametrize("kind", ["goac", "ptrain"])
def test_reference_unshared_checkpoint_round_trips_and_resumes(kind):
    """A checkpoint the reference trainer wrote with share_layers=False loads
    with weights_only=True, restores into the same keys, tensors and Adam
    state layout (lists of K state dicts, the separate std entries), comes
    back out of get_snapshot unchanged, and the next step matches the
    reference's (1e-5 on every tensor: no wider than the gate)."""
    fx = torch.load(os.path.join(HERE, "golden", f"{kind}_us_snapshot.pt"), weights_only=True)
    meta = dict(fx["meta"], soft=None)
    K = uo.n_critics(meta)
    tr = uo.trainer_for(meta)
    ref = fx["snapshot"]
    assert len(ref["qfs_state_dicts"]) == len(ref["qfs_optims_state_dicts"]) == K
    tr.restore_from_snapshot(ref)
    buf = io.BytesIO()
    torch.save(tr.get_snapshot(), buf)
    buf.seek(0)
    ours = torch.load(buf, weights_only=True)
    assert set(ours) == set(ref)
    for key in ("policy_state_dict", "target_policy_state_dict"):
        assert list(ours[key]) == list(ref[key])
        for k, v in ref[key].items():
            torch.testing.assert_close(_cpu(ours[key][k]), v, rtol=0, atol=0)
    for key in ("qfs_state_dicts", "target_qfs_state_dicts"):
        assert len(ours[key]) == K
        for i in range(K):
            assert list(ours[key][i]) == list(ref[key][i]) == uo.Q_ORDER
            for k, v in ref[key][i].items():
                torch.testing.assert_close(_cpu(ours[key][i][k]), v, rtol=0, atol=0)
    pairs = [(ours["policy_optim_state_dict"], ref["policy_optim_state_dict"]),
             (ours["target_policy_opt_state_dict"], ref["target_policy_opt_state_dict"])]
    pairs += list(zip(ours["qfs_optims_state_dicts"], ref["qfs_optims_state_dicts"]))
    for so_, sr in pairs:
        assert sorted(so_["state"]) == sorted(sr["state"])
        assert so_["param_groups"][0]["lr"] == sr["param_groups"][0]["lr"]
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
    mods = dict(policy=tr.policy, target_policy=tr.target_policy)
    for k in range(K):
        mods[f"qf{k}"], mods[f"tf{k}"] = tr.qfs[k], tr.tfs[k]
    worst = {}
    for grp, mod in mods.items():
        sd = mod.state_dict()
        for k, v in s3["post"][grp].items():
            worst[f"{grp}/{k}"] = parity.rel_err(_cpu(sd[k]).numpy(), v.numpy())
    print(sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    assert max(worst.values()) < TOL, worst


# -------------------------------------------------------------- entry paths
def _state(tr):
    torch.cuda.synchronize()
    return torch.cat([tr.params, tr.targets, tr.adam_m, tr.adam_v]).cpu().numpy()


@pytest.mark.parametrize("kind,K", [("goac", 2), ("ptrain", 10)])
def test_entry_paths_agree_bitwise(kind, K):
    """train_from_ring over 4 steps (and the drop-in random_batch + train call)
    against train_from_torch on the same minibatches, bit for bit."""
    from oac_amd import DeviceIndexStream, ReplayBuffer
    Do, Da, B, N = 1, 1, 32, 400
    meta = _meta(kind, Do, Da, 16, K=K, counts=False, lr=1e-3)
    data = synthetic_transitions(N, Do, Da, seed=1)

    def replay():
        rb = ReplayBuffer(N, Space(Do), Space(Da), device="cuda:0")
        rb.add_paths([dict(observations=data["observations"], actions=data["actions"],
                           rewards=data["rewards"], next_observations=data["next_observations"],
                           terminals=data["terminals"])])
        return rb

    tr, rb = uo.trainer_for(meta), replay()
    st = DeviceIndexStream(rb, B, chunk=8, seed=4)
    st.before_step(4)
    torch.cuda.synchronize()
    ring = st.ring.view(st.slots, B)[:4].cpu().numpy().astype(np.int64)
    tr.train_from_ring(rb._storage, st.ring, st.slots, B, n_steps=4)
    tr2 = uo.trainer_for(meta)
    for idx in ring:
        tr2.train_from_torch({k: v[idx] for k, v in data.items()})
    assert np.isfinite(_state(tr2)).all()
    np.testing.assert_array_equal(_state(tr), _state(tr2))
    assert tr._n_train_steps_total == 4
    tr3, rb3 = uo.trainer_for(meta), replay()
    np.random.seed(3)
    drawn = []
    for _ in range(3):
        batch = rb3.random_batch(B)
        drawn.append(np.array(batch.host_indices))
        batch["buffer"] = rb3
        tr3.train(batch)
    tr4 = uo.trainer_for(meta)
    for idx in drawn:
        tr4.train_from_torch({k: v[idx] for k, v in data.items()})
    np.testing.assert_array_equal(_state(tr3), _state(tr4))


# ------------------------------------------------------------- what raises
def test_unsupported_configurations_raise_by_name():
    from oac_amd import _lib
    m1 = _meta("goac", 5, 2, 24)
    for kw, names in ((dict(global_opt=True), ["global_opt"]), (dict(use_graph=True), ["use_graph"])):
        for meta in (m1, _meta("ptrain", 5, 2, 24, K=3)):
            with pytest.raises(NotImplementedError) as e:
                uo.trainer_for(meta, **kw)
            assert all(n in str(e.value) for n in names + ["share_layers=False"]), str(e.value)
    # two hidden layers with share_layers=False: both options named
    for kind, K in (("goac", 2), ("ptrain", 3)):
        m2 = dict(_meta(kind, 5, 2, 24, K=K), hidden=[24, 24])
        with pytest.raises(NotImplementedError) as e:
            uo.trainer_for(m2)
        assert "share_layers" in str(e.value) and "num_layers" in str(e.value), str(e.value)
    with pytest.raises(NotImplementedError, match="n_estimators"):
        uo.trainer_for(_meta("ptrain", 5, 2, 24, K=17))
    # the data-parallel trainers (before they touch the process group)
    pp, qp = uo.producers(uo.params_of(m1), "goac")
    from oac_amd.dp import DataParallelGaussianTrainer, DataParallelParticleTrainer
    for cls in (DataParallelGaussianTrainer, DataParallelParticleTrainer):
        with pytest.raises(NotImplementedError, match="share_layers"):
            cls(pp, qp, n_estimators=2, action_space=Space(2), share_layers=False)
    # the C ABI's single-process entry points on an unshared handle
    tr = uo.trainer_for(m1)
    b = _batch(5, 2, 16, 6)
    tr.train_from_torch(b)
    torch.cuda.synchronize()
    L, h = _lib.lib(), tr._last_plan.handle
    assert L.oac_sac_step(h, _lib.OAC_STEP_USE_GRAPH, None) != 0
    assert b"unshared" in L.oac_last_error() and b"OAC_STEP_USE_GRAPH" in L.oac_last_error()
    assert L.oac_sac_step_phase(h, 0, 0, None) != 0
    assert b"unshared" in L.oac_last_error() and b"oac_sac_step_phase" in L.oac_last_error()
    assert L.oac_sac_set_allreduce(h, None, None, 0) != 0
    assert b"unshared" in L.oac_last_error() and b"oac_sac_set_allreduce" in L.oac_last_error()


# --------------------------------- the shared-layer step through these kernels
@pytest.mark.parametrize("name", sl.FIXTURES)
def test_shared_step_ignores_the_new_fields_bitwise(name):
    """The shared-layer depth-1 fixtures through the kernels this feature
    changed (row_heads / row_heads2 with the segment width unset, the targets
    kernels, the seed kernel, the head launch): a trainer whose plans carry
    unshared = 0 and a stray std_lr ends bit-identical to the plain one, and
    its plan has the shared layout.  (The values themselves are held to the
    reference by the untouched test_gpu_shallow.py.)"""
    meta, g = parity.load(name)

    def run(std_lr):
        tr = sl.trainer_for(meta)
        assert not tr.unshared
        tr.std_lr = std_lr   # (reaches oac_sac_config.std_lr; no shared plan reads it)
        if meta.get("use_target_policy"):
            sl.load_tpn(tr, g)
        for s in range(meta["steps"]):
            b = batch_from(meta, g[f"s{s}/idx"])
            if meta["counts"]:
                b["counts"] = g[f"s{s}/counts"][:, None]
            tr.train_from_torch(b)
        cfg = tr._make_cfg(meta["B"])
        assert cfg.unshared == 0 and cfg.std_lr == std_lr
        assert tr.layout.n_critics == 1 and _launches(tr) == 8
        return _state(tr), torch.cat([tr.grads]).cpu().numpy()

    a, b = run(0.0), run(0.125)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
