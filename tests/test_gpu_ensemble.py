"""ParticleTrainer(ensemble=True, n_policies=P) on the GPU: the stacked-policy
step (csrc/det_plan.hip, csrc/ensemble.hip) against the reference's own
ensemble runs (tests/golden/ens_*.npz) and the CPU oracle
(tests/ensemble_oracle.py), acting (oac_ensemble_eval) against the reference's
recorded choices, a shape sweep from a mid-training state, the launch count,
the reference's interface and snapshots, the configurations that must raise,
and the w_oac no-resampling recipe's loop."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import parity
import test_oracle_golden as tog
from gpu_helpers import batch_from, module_tensors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5
DEV = "cuda:0"


def _launches(tr):
    from oac_amd import _lib
    return _lib.lib().oac_sac_launch_count(tr._last_plan.handle)


def _view(tr, name):
    torch.cuda.synchronize()
    return tr._last_plan.views[name].detach().cpu().numpy()


def _forced_step(tr, meta, b):
    """One GPU step and the fp32 oracle's step from the same pre-step state:
    (errors, the oracle's outputs); the chosen indices and the selection's
    margins are checked here."""
    orc = eo.oracle_from_gpu(tr, meta)
    out = orc.step(b)
    tr.train_from_torch(b)
    errs = eo.step_errors_against_oracle(tr, orc, out, meta)
    assert out["min_gap"] >= eo.MIN_GAP, out["min_gap"]
    if out["sel"] is not None:
        assert out["sel_gap"] >= eo.MIN_GAP, out["sel_gap"]
        assert np.array_equal(_view(tr, "ens_sel")[:, 0].astype(np.int64), out["sel"].numpy())
        errs["ub_next"] = parity.rel_err(_view(tr, "ens_ub_next").T, out["ub_next"].numpy())
    else:
        assert _view(tr, "ens_sel").size == 0
    errs["tq"] = parity.rel_err(_view(tr, "tq1").T, out["tq"].numpy())
    errs["ub_obs"] = parity.rel_err(_view(tr, "ens_ub_obs").T, out["upper_bounds"].numpy())
    errs["qnew"] = parity.rel_err(_view(tr, "qnew")[:, 0], out["upper_bound"].numpy())
    P, Da = meta["P"], meta["act_dim"]
    acts = _view(tr, "ens_act").reshape(-1, P, Da).transpose(1, 0, 2)
    errs["obs_actions"] = parity.rel_err(acts, out["obs_actions"].numpy())
    return errs, out


# ------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("name", eo.FIXTURES)
def test_step_matches_reference_and_oracle(name):
    """Per fixture and per step, nothing left out: (teacher-forced) from the
    GPU trainer's own pre-step state every network's gradient, post-step
    parameters, Adam m / v and target within 1e-5 of the fp32 oracle's step and
    the chosen indices equal; along the trajectory the same quantities, the
    target critics' values and the statistics (keys in the reference's order)
    against the reference's recording under the project's gate, the recorded
    chosen indices equal."""
    meta, g = parity.load(name)
    tr = eo.trainer_for(meta)
    P, K = meta["P"], meta["K"]
    assert tr.n_hidden == 1 and tr.unshared and tr.ensemble
    assert len(tr.policy.policies) == len(tr.policy_optimizers) == P
    errs, forced = {}, {}
    for s in range(meta["steps"]):
        tr.end_epoch(s)
        b = batch_from(meta, g[f"s{s}/idx"])
        if meta["counts"]:
            b["counts"] = g[f"s{s}/counts"][:, None]
        fe, out = _forced_step(tr, meta, b)
        forced.update({f"s{s}/{k}": v for k, v in fe.items()})
        if not meta["mean_update"]:
            assert np.array_equal(_view(tr, "ens_sel")[:, 0].astype(np.int64), g[f"s{s}/sel"])
        errs[f"s{s}/tq"] = parity.compare(g, f"s{s}/tq", _view(tr, "tq1").T)
        groups = [(f"policy{p}", eo.POL_ORDER) for p in range(P)] + [("target_policy", eo.POL_ORDER)]
        groups += [(f"qf{k}", eo.Q_ORDER) for k in range(K)]
        for grp, order in groups:
            mod = eo.gpu_module(tr, grp)
            assert list(mod.state_dict()) == order
            gv = module_tensors(tr, mod, tr.grads)
            mv, vv = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
            sd = mod.state_dict()
            for pn in order:
                key = f"s{s}/grad/{grp}/{pn}"
                errs[key] = parity.compare(g, key, gv[pn].cpu().numpy())
                key = f"s{s}/post/{grp}/{pn}"
                gk = f"s{s}/grad/{grp}/{pn}" if s == 0 else None
                errs[key], _ = parity.compare_post(g, key, gk, sd[pn].cpu().numpy(), meta["lr"])
                errs[f"s{s}/adam_m/{grp}/{pn}"] = parity.compare(g, f"s{s}/adam_m/{grp}/{pn}",
                                                                 mv[pn].cpu().numpy())
                errs[f"s{s}/adam_v/{grp}/{pn}"] = parity.compare(g, f"s{s}/adam_v/{grp}/{pn}",
                                                                 vv[pn].cpu().numpy())
        for k in range(K):
            for pn, t in tr.tfs[k].state_dict().items():
                errs[f"s{s}/post/tf{k}/{pn}"] = parity.compare(g, f"s{s}/post/tf{k}/{pn}",
                                                               t.cpu().numpy())
        keys = [k[len(f"s{s}/stat/"):] for k in g if k.startswith(f"s{s}/stat/")]
        assert list(tr.get_diagnostics().keys()) == keys
        for k, v in tr.get_diagnostics().items():
            errs[f"s{s}/stat/{k}"] = parity.stat_err(v, g, f"s{s}/stat/{k}")
    print(name, "teacher-forced worst", sorted(forced.items(), key=lambda kv: -kv[1])[:3])
    print(name, "trajectory worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    bad = {k: v for k, v in forced.items() if v > TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:10]
    noise = eo.oracle_errors(meta, g, torch.float64)
    assert set(noise) <= set(errs)
    bad = tog.gated(errs, noise)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]
    # every optimizer stepped once per train step; the log-std heads keep no state
    for opt in tr.policy_optimizers + [tr.target_policy_optimizer]:
        st = opt.state_dict()["state"]
        assert sorted(st) == [0, 1, 2, 3] and all(v["step"] == meta["steps"] for v in st.values())
    assert tr.policy_optimizer.state_dict()["state"] == {}


# ------------------------------------------------------- 2. acting, evaluation
def _acting_trainer():
    """The ragged fixture's trainer in the state the reference recorded its 64
    observations on (the final step's parameters)."""
    meta, g = parity.load("ens_ragged")
    tr = eo.trainer_for(meta)
    s = meta["steps"] - 1
    sd = lambda grp, order: {pn: torch.from_numpy(g[f"s{s}/post/{grp}/{pn}"]) for pn in order}
    tr.policy.load_state_dict([sd(f"policy{p}", eo.POL_ORDER) for p in range(meta["P"])])
    for k, q in enumerate(tr.qfs):
        q.load_state_dict(sd(f"qf{k}", eo.Q_ORDER))
    return meta, g, tr


def test_acting_matches_the_reference_record():
    meta, g, tr = _acting_trainer()
    obs, Da = g["act/obs"], meta["act_dim"]
    six = tr.policy.forward(torch.from_numpy(obs).float().to(DEV), deterministic=True)
    torch.cuda.synchronize()
    assert np.array_equal(tr.policy.last_choice.cpu().numpy(), g["act/sel"])
    assert parity.rel_err(tr.policy.last_upper_bounds.cpu().numpy().T, g["act/ub"]) < TOL
    for t, nm in zip(six, ("action", "mean", "log_std", "log_prob", "std", "pre_tanh")):
        assert tuple(t.shape) == (64, Da), nm
        assert parity.rel_err(t.cpu().numpy(), g[f"act/forward/{nm}"]) < TOL, nm
    best = tr.policy.get_best_actions(obs, deterministic=True)
    assert np.array_equal(tr.policy.last_choice.cpu().numpy(), g["act/sel"])
    assert best.shape == (64, Da) and parity.rel_err(best, g["act/get_action"]) < TOL
    for i in range(0, 64, 7):   # get_action: one observation per call
        a, info = tr.policy.get_action(obs[i], deterministic=True)
        assert info == {} and a.shape == (Da,)
        assert int(tr.policy.last_choice.cpu()[0]) == int(g["act/sel"][i])
        assert parity.rel_err(a, g["act/get_action"][i]) < TOL
    one = tr.policy.forward(torch.from_numpy(obs[3]).float().to(DEV), deterministic=True)
    assert all(tuple(t.shape) == (Da,) for t in one)
    assert torch.equal(one[0], six[0][3])
    # get_actions(index=i): policy i's own module; its predict is the recorded upper bound
    for i in range(meta["P"]):
        a = tr.policy.get_actions(obs, deterministic=True, index=i)
        assert np.array_equal(a, tr.policy.policies[i].get_actions(obs, deterministic=True))
        assert parity.rel_err(a, g["act/proposals"][i]) < TOL
        assert parity.rel_err(tr.predict(obs, a).cpu().numpy()[:, 0], g["act/ub"][i]) < TOL


def test_sampled_acting_equals_the_oracle_for_a_fixed_noise():
    meta, g, tr = _acting_trainer()
    obs = g["act/obs"]
    noise = np.random.RandomState(4).standard_normal((64, meta["P"], meta["act_dim"])).astype(np.float32)
    orc = eo.oracle_from_gpu(tr, meta)
    want = orc.act(obs, noise)
    assert want["sel_gap"] >= eo.MIN_GAP and len(set(want["sel"].tolist())) >= 2
    six = tr.policy.forward(torch.from_numpy(obs).float().to(DEV), deterministic=False,
                            return_log_prob=True, noise=noise)
    torch.cuda.synchronize()
    assert np.array_equal(tr.policy.last_choice.cpu().numpy(), want["sel"].numpy())
    assert tuple(six[3].shape) == (64, 1)
    for t, nm in zip(six, ("action", "mean", "log_std", "log_prob", "std", "pre_tanh")):
        assert parity.rel_err(t.cpu().numpy(), want[nm].numpy()) < TOL, nm
    a = tr.policy.get_best_actions(obs, deterministic=False, noise=noise)
    assert parity.rel_err(a, want["action"].numpy()) < TOL
    # without a given noise every call draws its own
    b1 = tr.policy.get_best_actions(obs, deterministic=False)
    b2 = tr.policy.get_best_actions(obs, deterministic=False)
    assert np.isfinite(b1).all() and not np.array_equal(b1, b2)


# ------------------------------------------------------------- 3. shape sweep
@pytest.mark.parametrize("name", sorted(eo.SWEEP))
def test_one_step_from_a_mid_training_state(name):
    """WARMUP steps, then one step from the trainer's own state (Adam step > 0,
    moments nonzero) against the fp32 oracle: every tensor whole within 1e-5,
    the chosen indices equal."""
    meta, B = eo.SWEEP[name]
    kw = {}
    tr = eo.trainer_for(meta, **kw)
    assert tr.delta_index == meta["delta_index"]
    for s in range(eo.WARMUP):
        tr.train_from_torch(eo.sweep_batch(meta, B, 6 + s))
    torch.cuda.synchronize()
    assert tr._n_train_steps_total == eo.WARMUP and float(tr.adam_m.abs().sum()) > 0
    errs, out = _forced_step(tr, meta, eo.sweep_batch(meta, B, 6 + eo.WARMUP))
    print(name, sorted(errs.items(), key=lambda kv: -kv[1])[:3], _launches(tr))
    bad = {k: v for k, v in errs.items() if v > TOL}
    assert not bad, bad
    assert _launches(tr) == (12 if B < 512 else 14)   # (slab reduction, unfused policy Adam)


# ------------------------------------------------------------ 4. launch count
@pytest.mark.parametrize("mean_update", [False, True])
def test_launch_count_does_not_depend_on_n_policies(mean_update):
    """Small batch, batch given: 12 launches (the count DESIGN.md records),
    whatever P -- three more than the unshared step without the ensemble."""
    import unshared_oracle as uo
    counts = []
    for P in (2, 16):
        meta = eo.sweep_meta(2, 1, 16, P, 10, mean_update=mean_update)
        tr = eo.trainer_for(meta)
        tr.train_from_torch(eo.sweep_batch(meta, 32, 6))
        torch.cuda.synchronize()
        counts.append(_launches(tr))
    assert counts == [12, 12]
    plain = uo.trainer_for(dict(meta, soft=None), mean_update=mean_update)
    plain.train_from_torch(eo.sweep_batch(meta, 32, 6))
    torch.cuda.synchronize()
    assert _launches(plain) == 9


# ---------------------------------------------------------------- 5. interface
def _tstate(tr):
    torch.cuda.synchronize()
    return torch.cat([tr.params, tr.targets, tr.adam_m, tr.adam_v]).cpu().numpy()


def test_objects_producer_calls_and_the_initial_action_draw():
    """particle_trainer.py:115-137: the ensemble producer call after the K
    critics with the constructor's initial actions -- for act_dim > 1 drawn on
    numpy's global stream, which advances exactly as in the reference."""
    meta, g = parity.load("ens_ragged")
    np.random.seed(meta["np_seed"])
    tr = eo.trainer_for(meta)
    after = np.random.uniform()
    rs = np.random.RandomState(meta["np_seed"])
    rs.uniform(-1, 1, (meta["P"], meta["act_dim"]))
    assert after == rs.uniform()
    calls = tr.policy_producer_calls
    assert [bool(c.get("ensemble")) for c in calls] == [False, True, False]
    c = calls[1]
    assert np.allclose(c["bias"], meta["initial_actions"], rtol=1e-6, atol=0)
    assert c["n_policies"] == meta["P"] and c["approximator"] is tr and c["share_layers"] is False
    pols = tr.policy.policies
    assert tr.networks == pols + tr.qfs + tr.tfs + [tr.target_policy]
    assert tr.policy.n_policies == 3 and tr.policy.share_layers is False
    assert tr.policy.approximator is tr
    assert tr.optimize_policies(None) is None
    # policy p is slice p of the stacked block
    E, H, Do, Da = tr.ens_layout, 24, 5, 3
    base = tr.params.data_ptr()
    for p, pol in enumerate(pols):
        assert list(pol.state_dict()) == eo.POL_ORDER
        assert pol.fc0.weight.data_ptr() == base + 4 * (E.ens_fc0_w + p * H * Do)
        assert pol.fc0.bias.data_ptr() == base + 4 * (E.ens_fc0_b + p * H)
        assert pol.last_fc.weight.data_ptr() == base + 4 * (E.ens_head_w + p * 2 * Da * H)
        assert pol.last_fc_log_std.bias.data_ptr() == base + 4 * (E.ens_head_b + p * 2 * Da + Da)
    assert tr.target_policy.fc0.weight.data_ptr() == base + 4 * tr.layout.tpol_base
    m1, _ = parity.load("ens_plain")
    t1 = eo.trainer_for(m1)
    assert t1.initial_actions.tolist() == m1["initial_actions"]
    sds = tr.policy.state_dict()
    assert isinstance(sds, list) and len(sds) == 3
    tr.policy.load_state_dict(sds)
    tr.policy.reset()
    tr.policy.to(device=DEV)


def test_snapshot_round_trip_is_bitwise():
    meta, g = parity.load("ens_counts")

    def batch(s):
        b = batch_from(meta, g[f"s{s}/idx"])
        b["counts"] = g[f"s{s}/counts"][:, None]
        return b
    a = eo.trainer_for(meta)
    for s in range(2):
        a.train_from_torch(batch(s))
    snap = a.get_snapshot()
    assert isinstance(snap["policy_state_dict"], list) and len(snap["policy_state_dict"]) == 5
    assert snap["policy_optim_state_dict"]["state"] == {}
    assert len(snap["policy_optims_state_dicts"]) == 5
    buf = io.BytesIO()
    torch.save(snap, buf)
    b = eo.trainer_for(meta)
    buf.seek(0)
    b.restore_from_snapshot(torch.load(buf, weights_only=False))
    np.testing.assert_array_equal(_tstate(a).view(np.uint32), _tstate(b).view(np.uint32))
    assert b._n_train_steps_total == 2
    for oa, ob in zip(a.policy_optimizers, b.policy_optimizers):
        assert [v["step"] for v in oa.state_dict()["state"].values()] == \
            [v["step"] for v in ob.state_dict()["state"].values()] == [2] * 4
    a.train_from_torch(batch(2))
    b.train_from_torch(batch(2))
    np.testing.assert_array_equal(_tstate(a).view(np.uint32), _tstate(b).view(np.uint32))


def test_reference_written_snapshot_loads_and_resumes():
    """The reference's checkpoint has the list of P policy state dicts and the
    never-stepped parent optimizer, and no per-policy optimizer entry: it
    restores with the policies' moments left as they are -- here set to the
    moments the reference held, recorded beside the checkpoint -- and the next
    step matches the oracle and the reference's own third step."""
    fx = torch.load(os.path.join(HERE, "golden", "ens_snapshot.pt"), weights_only=True)
    meta = dict(fx["meta"], soft=None)
    tr = eo.trainer_for(meta)
    ref = fx["snapshot"]
    assert "policy_optims_state_dicts" not in ref and len(ref["policy_state_dict"]) == meta["P"]
    tr.restore_from_snapshot(ref)
    assert tr._n_train_steps_total == 2
    assert set(tr.get_snapshot()) == set(ref) | {"policy_optims_state_dicts"}
    for p, pol in enumerate(tr.policy.policies):
        for k, v in ref["policy_state_dict"][p].items():
            assert torch.equal(pol.state_dict()[k].cpu(), v)
    assert float(sum(m.abs().sum() for o in tr.policy_optimizers for m in o.m)) == 0.0
    for opt, moms in zip(tr.policy_optimizers, fx["policy_moments"]):
        for i, mv in enumerate(moms):
            if mv is not None:
                opt.m[i].copy_(mv["m"].reshape(opt.m[i].shape))
                opt.v[i].copy_(mv["v"].reshape(opt.v[i].shape))
    s3 = fx["step3"]
    b = batch_from(meta, s3["idx"].numpy())
    errs, _ = _forced_step(tr, meta, b)
    bad = {k: v for k, v in errs.items() if v > TOL}
    assert not bad, bad
    torch.cuda.synchronize()
    worst = {}
    for grp, post in s3["post"].items():
        mod = tr.tfs[int(grp[2:])] if grp.startswith("tf") else eo.gpu_module(tr, grp)
        for k, v in post.items():
            worst[f"{grp}/{k}"] = parity.rel_err(mod.state_dict()[k].cpu().numpy(), v.numpy())
    print(sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    assert max(worst.values()) < 1e-4   # (three fp32 steps of Adam's lr * sign(g) apart at most)


def test_rejections_name_every_offending_option():
    import oac_amd
    from oac_amd import dp
    meta, _ = parity.load("ens_plain")
    cases = [(dict(share_layers=True), ["share_layers"]),
             (dict(global_opt=True), ["global_opt"]),
             (dict(use_graph=True), ["use_graph"]),
             (dict(use_target_policy=True), ["use_target_policy"]),
             (dict(mellow_max=True), ["mellow_max"]),
             (dict(n_policies=0), ["n_policies"]),
             (dict(n_policies=17), ["n_policies"]),
             (dict(global_opt=True, use_graph=True, mellow_max=True),
              ["global_opt", "use_graph", "mellow_max"])]
    for kw, names in cases:
        with pytest.raises(NotImplementedError) as e:
            eo.trainer_for(meta, **kw)
        assert "ensemble" in str(e.value) and all(n in str(e.value) for n in names), (kw, str(e.value))
    eo.trainer_for(meta, use_target_policy=True, mean_update=True)   # (the reference accepts it)
    # two hidden layers
    m2 = dict(meta, hidden=[16, 16])
    p2 = eo.params_of(m2)
    with pytest.raises(NotImplementedError) as e:
        eo.trainer_for(m2, params=p2)
    assert "ensemble" in str(e.value) and "num_layers" in str(e.value)
    pp, qp = eo.producers(eo.params_of(meta))
    with pytest.raises(NotImplementedError, match="ensemble"):
        oac_amd.GaussianTrainer(pp, qp, action_space=eo.Space(1), ensemble=True)
    with pytest.raises(NotImplementedError, match="ensemble"):
        oac_amd.ParticleTrainerOAC(pp, qp, n_estimators=10, action_space=eo.Space(1),
                                   share_layers=True, ensemble=True)
    with pytest.raises(NotImplementedError, match="ensemble"):
        dp.DataParallelParticleTrainer(pp, qp, n_estimators=10, action_space=eo.Space(1),
                                       ensemble=True, n_policies=5)


def test_handle_refuses_graph_phase_and_allreduce_by_name():
    from oac_amd import _lib
    L = _lib.lib()
    meta, g = parity.load("ens_plain")
    tr = eo.trainer_for(meta)
    tr.train_from_torch(batch_from(meta, g["s0/idx"]))
    torch.cuda.synchronize()
    before = _tstate(tr)
    h = tr._last_plan.handle
    sp = _lib.stream_ptr(tr.stream)
    assert L.oac_sac_step(h, _lib.OAC_STEP_USE_GRAPH, sp) != 0
    assert b"ensemble" in L.oac_last_error() and b"OAC_STEP_USE_GRAPH" in L.oac_last_error()
    assert L.oac_sac_step_phase(h, 0, 0, sp) != 0
    assert b"ensemble" in L.oac_last_error() and b"oac_sac_step_phase" in L.oac_last_error()
    assert L.oac_sac_set_allreduce(h, None, None, 0) != 0
    assert b"ensemble" in L.oac_last_error() and b"oac_sac_set_allreduce" in L.oac_last_error()
    np.testing.assert_array_equal(before.view(np.uint32), _tstate(tr).view(np.uint32))


# ------------------------------------------------------------ 6. recipe loop
def test_drop_in_path_equals_train_from_torch():
    """random_batch of an ordinary device ReplayBuffer (host indices staged
    through the plan's ring, the gather inside the step) against the same rows
    given as a batch: bitwise, 3 steps; one launch more (the gather)."""
    from noresample_oracle import make_path
    from oac_amd import ReplayBuffer
    meta, _ = parity.load("ens_plain")
    a, b = eo.trainer_for(meta), eo.trainer_for(meta)
    rb = ReplayBuffer(300, eo.Space(2), eo.Space(1), device=DEV)
    rb.add_path(make_path(np.random.RandomState(3), 300, 2, 1))
    r = rb.rows
    np.random.seed(9)
    for _ in range(3):
        batch = rb.random_batch(32)
        assert batch.host_indices is not None
        rows = rb._storage[torch.as_tensor(batch.host_indices, device=DEV)].cpu().numpy()
        batch["buffer"] = rb
        a.train(batch)
        col = lambda o, n: rows[:, o:o + n]
        b.train_from_torch(dict(observations=col(r["off_obs"], 2), actions=col(r["off_act"], 1),
                                rewards=col(r["off_rew"], 1), terminals=col(r["off_term"], 1),
                                next_observations=col(r["off_next_obs"], 2)))
    np.testing.assert_array_equal(_tstate(a).view(np.uint32), _tstate(b).view(np.uint32))
    assert (_launches(a), _launches(b)) == (13, 12)


class _StubEnv:
    """A deterministic 2-d environment: enough for path_collector's loop."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def reset(self):
        self.o = self.rs.uniform(-1, 1, 2)
        return self.o

    def step(self, a):
        self.o = np.clip(self.o + 0.1 * float(np.asarray(a).reshape(-1)[0]), -2, 2)
        return self.o, float(-abs(self.o[0])), False, {}


def test_no_resampling_recipe_loop():
    """w_oac_mountain_no_resampling.sh's construction (--alg p-oac --ensemble
    --no_resampling --num_layers 1 --layer_size 16 --n_estimators 10, n_policies
    5) with oac_amd's producers and device ReplayBufferNoResampling: 20 steps of
    random_batch + train at B 32 with paths added as the loop goes, bitwise
    equal to train_from_torch on the same rows; then vec_rollout over 4
    environments acts through get_best_actions."""
    import oac_amd
    from noresample_oracle import make_path
    from oac_amd import ReplayBufferNoResampling, get_policy_producer, get_q_producer, vec_rollout

    def build():
        torch.manual_seed(0)
        np.random.seed(0)
        pp = get_policy_producer(2, 1, [16], device=DEV)
        qp = get_q_producer(2, 1, [16], device=DEV)
        return oac_amd.ParticleTrainer(
            pp, qp, n_estimators=10, action_space=eo.Space(1), delta=0.95, q_min=0, q_max=100,
            ensemble=True, n_policies=5, share_layers=False, deterministic=True, discount=0.99,
            soft_target_tau=5e-3, target_update_period=1, policy_lr=3e-4, qf_lr=3e-4,
            use_automatic_entropy_tuning=True)
    a, b = build(), build()
    np.testing.assert_array_equal(_tstate(a).view(np.uint32), _tstate(b).view(np.uint32))
    B, N = 32, 2000
    rb = ReplayBufferNoResampling(N, eo.Space(2), eo.Space(1), device=DEV, index_source="device",
                                  seed=5)
    rs = np.random.RandomState(3)
    rb.add_path(make_path(rs, 320, 2, 1))
    r = rb.rows
    for step in range(20):
        if step % 5 == 4:
            rb.add_path(make_path(rs, 160, 2, 1))
        batch = rb.random_batch(B)
        batch["buffer"] = rb
        torch.cuda.synchronize()
        rows = rb._storage[batch.indices.long()].cpu().numpy()
        a.train(batch)
        col = lambda o, n: rows[:, o:o + n]
        b.train_from_torch(dict(observations=col(r["off_obs"], 2), actions=col(r["off_act"], 1),
                                rewards=col(r["off_rew"], 1), terminals=col(r["off_term"], 1),
                                next_observations=col(r["off_next_obs"], 2)))
    sa, sb = _tstate(a), _tstate(b)
    assert np.isfinite(sa).all() and a._n_train_steps_total == 20
    np.testing.assert_array_equal(sa.view(np.uint32), sb.view(np.uint32))
    assert all(np.isfinite(v) for v in a.get_diagnostics().values())
    paths = vec_rollout([_StubEnv(i) for i in range(4)], a.policy, max_path_length=10,
                        deterministic_pol=True)
    assert len(paths) == 4
    for p in paths:
        assert p["actions"].shape == (10, 1) and np.isfinite(p["actions"]).all()
        assert np.abs(p["actions"]).max() <= 1.0
        want = a.policy.get_action(p["observations"][3], deterministic=True)[0]
        assert np.array_equal(want, p["actions"][3])
    # the evaluation wrapper acts through the same best-of-P call
    wrapped = vec_rollout([_StubEnv(i) for i in range(4)], oac_amd.MakeDeterministic(a.policy),
                          max_path_length=10)
    for p, w in zip(paths, wrapped):
        assert np.array_equal(p["actions"], w["actions"])
