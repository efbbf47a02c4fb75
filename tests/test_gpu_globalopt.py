"""``global_opt`` for the g-oac GaussianTrainer and the p-oac ParticleTrainer
on the GPU: the train step that leaves the policy alone and the policy sweep
``optimize_policies`` (csrc/det_plan.hip, the policy-only Adam of
csrc/adam.hip) against the reference's own runs (tests/golden/*_go_*.npz) and
the CPU restatement (tests/globalopt_lib.py); determinism, buffers, plans,
snapshots and errors.  Every case has N <= 1300 rows."""
import io
import random

import numpy as np
import pytest
import torch

import globalopt_lib as gl
import parity
import shallow_lib as sl
import test_oracle_golden as tog
from fixtures_lib import synthetic_transitions
from gpu_helpers import Space, batch_from, module_tensors

pytestmark = pytest.mark.gpu


def _buffer(Do, Da, n, capacity=None, seed=0):
    """An oac_amd.ReplayBuffer holding the n synthetic transitions."""
    import oac_amd
    rb = oac_amd.ReplayBuffer(capacity or n + 8, Space(Do), Space(Da))
    tr = synthetic_transitions(n, Do, Da, seed=seed)
    rb.load_transitions(torch.from_numpy(rb._rows_from(
        tr["observations"], tr["actions"], tr["rewards"], tr["next_observations"],
        tr["terminals"])))
    return rb


def _fixture_buffer(meta, **kw):
    return _buffer(meta["obs_dim"], meta["act_dim"], meta["n_replay"], **kw)


def _block(tr, arena):
    return arena[:int(tr.layout.pol_size)].clone()


def _launches(tr):
    from oac_amd import _lib
    return _lib.lib().oac_sac_launch_count(tr._last_plan.handle)


def _train(tr, meta, g, s):
    tr.end_epoch(s)
    b = batch_from(meta, g[f"s{s}/idx"])
    if meta["counts"]:
        b["counts"] = g[f"s{s}/counts"][:, None]
    tr.train_from_torch(b)
    torch.cuda.synchronize()


_RUNS = {}


def _run(name):
    """The fixture's whole sequence on the GPU, once per fixture: errors of
    everything the reference recorded, and what the other checks need."""
    if name in _RUNS:
        return _RUNS[name]
    meta, g = parity.load(name)
    tr = gl.trainer_for(meta)
    plain = gl.trainer_for(meta, global_opt=False)
    qf, tf = sl.critic_of(tr)
    pol_order, q_order = sl.orders(len(meta["hidden"]))
    rb = _fixture_buffer(meta)
    random.seed(meta["rseed"])
    errs, rec = {}, dict(untouched=[], stat_keys=[], launches=[], restart=[], steps=[], hist=[])
    s = c = 0
    for what, n in gl.SEQUENCE:
        if what == "train":
            for _ in range(n):
                before = [_block(tr, a) for a in (tr.params, tr.adam_m, tr.adam_v)]
                _train(tr, meta, g, s)
                rec["untouched"].append(all(torch.equal(x, _block(tr, a)) for x, a in zip(
                    before, (tr.params, tr.adam_m, tr.adam_v))))
                for grp, mod, order in (("target_policy", tr.target_policy, pol_order),
                                        ("qf", qf, q_order)):
                    gv = module_tensors(tr, mod, tr.grads)
                    for pn in order:
                        key = f"s{s}/grad/{grp}/{pn}"
                        errs[key] = parity.compare(g, key, gv[pn].cpu().numpy())
                for grp, mod in (("policy", tr.policy), ("target_policy", tr.target_policy),
                                 ("qf", qf), ("tf", tf)):
                    for pn, t in mod.state_dict().items():
                        key = f"s{s}/post/{grp}/{pn}"
                        gk = f"s{s}/grad/{grp}/{pn}" if s == 0 and grp in ("target_policy", "qf") \
                            else None
                        errs[key], _ = parity.compare_post(g, key, gk, t.cpu().numpy(), meta["lr"])
                rec["stat_keys"].append((list(tr.get_diagnostics().keys()),
                                         [str(k) for k in g[f"s{s}/stat_keys"]]))
                for k, v in tr.get_diagnostics().items():
                    errs[f"s{s}/stat/{k}"] = parity.stat_err(v, g, f"s{s}/stat/{k}")
                if s == 0:   # the same step without global_opt: its launch count
                    _train(plain, meta, g, 0)
                    rec["launches"] = [_launches(tr), _launches(plain)]
                s += 1
            continue
        m0 = _block(tr, tr.adam_m)
        tr.optimize_policies(rb, iterations=n)
        torch.cuda.synchronize()
        assert len(tr.policy_opt_history["loss"]) == n
        for k in range(n):
            errs[f"c{c}/i{k}/loss"] = parity.rel_err(
                np.array([tr.policy_opt_history["loss"][k]]), g[f"c{c}/i{k}/loss"])
            errs[f"c{c}/i{k}/grad_norm"] = parity.rel_err(
                np.array([tr.policy_opt_history["grad_norm"][k]]), g[f"c{c}/i{k}/grad_norm"])
        gv = module_tensors(tr, tr.policy, tr.grads)   # the call's last iteration
        mv = module_tensors(tr, tr.policy, tr.adam_m)
        vv = module_tensors(tr, tr.policy, tr.adam_v)
        for pn, t in tr.policy.state_dict().items():
            key = f"c{c}/i{n - 1}/grad/policy/{pn}"
            errs[key] = parity.compare(g, key, gv[pn].cpu().numpy())
            errs[f"c{c}/post/policy/{pn}"] = parity.compare(g, f"c{c}/post/policy/{pn}",
                                                            t.cpu().numpy())
            if pn in gl.LOG_STD:
                assert not mv[pn].any() and not vv[pn].any()
                continue
            for nm, view in (("exp_avg", mv), ("exp_avg_sq", vv)):
                key = f"c{c}/opt/{nm}/{pn}"
                errs[key] = parity.compare(g, key, view[pn].cpu().numpy())
        rec["restart"].append(bool(m0.any()))   # moments entering the call (second: nonzero)
        st = lambda o: sorted({v["step"] for v in o.state_dict()["state"].values()})
        rec["steps"].append((st(tr.policy_optimizer), st(tr.target_policy_optimizer),
                             st(tr.qf_optimizers[0]), int(g[f"c{c}/opt/step"]),
                             int(tr._popt_state[0].item())))
        c += 1
    noise = gl.restatement_errors(meta, g, torch.float64)
    _RUNS[name] = (meta, errs, noise, rec, tr)
    return _RUNS[name]


def _gate(errs, noise, pick):
    sel = {k: v for k, v in errs.items() if pick(k)}
    assert sel
    print("worst", sorted(sel.items(), key=lambda kv: -kv[1])[:3])
    bad = tog.gated(sel, noise)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


# ------------------------------------------------- 1. train steps, goldens
@pytest.mark.parametrize("name", gl.FIXTURES)
def test_train_steps_leave_the_policy_alone(name):
    meta, errs, noise, rec, _ = _run(name)
    assert rec["untouched"] == [True] * meta["steps"]      # params / adam_m / adam_v, bitwise
    _gate(errs, noise, lambda k: k.startswith("s"))
    for got, want in rec["stat_keys"]:
        assert got == want and "Policy Loss" not in got
    assert rec["launches"][0] <= rec["launches"][1], rec["launches"]


# ------------------------------------------------ 2. the sweep, goldens
@pytest.mark.parametrize("name", gl.FIXTURES)
def test_first_iteration_gradient(name):
    meta, g = parity.load(name)
    tr = gl.trainer_for(meta)
    for s in range(2):
        _train(tr, meta, g, s)
    random.seed(meta["rseed"])
    tr.optimize_policies(_fixture_buffer(meta), iterations=1)
    torch.cuda.synchronize()
    gv = module_tensors(tr, tr.policy, tr.grads)
    errs = {f"c0/i0/grad/policy/{pn}": parity.compare(g, f"c0/i0/grad/policy/{pn}",
                                                      gv[pn].cpu().numpy()) for pn in gv}
    for k in ("loss", "grad_norm"):
        errs[f"c0/i0/{k}"] = parity.rel_err(np.array([tr.policy_opt_history[k][0]]),
                                            g[f"c0/i0/{k}"])
    _gate(errs, gl.restatement_errors(meta, g, torch.float64), lambda k: True)
    assert tr.policy_optimizer.state_dict()["state"][0]["step"] == 1
    # the global random stream is where one reference shuffle of N rows leaves it
    st = random.getstate()
    random.seed(meta["rseed"])
    gl.reference_shuffle_indices(meta["n_replay"], 1)
    assert random.getstate() == st


@pytest.mark.parametrize("name", gl.FIXTURES)
def test_sweep_sequence_matches_reference_golden(name):
    meta, errs, noise, rec, tr = _run(name)
    _gate(errs, noise, lambda k: k.startswith("c"))
    # (policy, target_policy, critic, fixture, device counter) step counts
    assert rec["steps"][0] == ([4], [2], [2], 4, 4)
    assert rec["steps"][1] == ([7], [3], [3], 7, 7)
    # the second call restarted the parameters from init_policy (its post
    # parameters are gated above) with the first call's moments carried on
    assert rec["restart"] == [False, True]
    assert tr.policy_opt_history.keys() == {"loss", "grad_norm"}


# --------------------------------------- 3. shuffle="none" vs restatement
def _meta(kind, Do, Da, hidden, K=2, **kw):
    m = dict(kind=kind, obs_dim=Do, act_dim=Da, hidden=hidden, K=K, seed=3, q_min=0.0,
             q_max=50.0, pi_init_w=0.2, q_init_w=0.1, discount=0.99, delta=0.95, lr=3e-4,
             tau=5e-3, counts=False)
    m.update(kw)
    return m


def _identity_against_restatement(tr, meta, rb, N, calls=(1, 2)):
    """shuffle='none' calls of 1 and then 2 iterations, each from the state the
    trainer is in (zero moments, then carried ones): the call's last policy
    gradient within 1e-5 (norm-relative, as test_gpu_ragged.py) of the
    restatement's, and every iteration's loss and grad norm."""
    if meta["kind"] == "ptrain":
        meta = dict(meta, delta_index=tr.delta_index)
    rs = gl.Restatement(meta)
    data = rb.get_dataset()
    data = (data.cpu().numpy() if torch.is_tensor(data) else np.asarray(data))[:N]
    worst = {}
    for it in calls:
        for k, v in rs.orc.opt_p.m.items():   # the optimizer state entering the call
            v.copy_(module_tensors(tr, tr.policy, tr.adam_m)[k].cpu())
            rs.orc.opt_p.v[k].copy_(module_tensors(tr, tr.policy, tr.adam_v)[k].cpu())
        rs.orc.opt_p.t = tr._policy_opt_steps
        want = rs.sweep(data, [np.arange(N)] * it)
        tr.optimize_policies(rb, iterations=it, shuffle="none")
        torch.cuda.synchronize()
        gv = module_tensors(tr, tr.policy, tr.grads)
        for pn in sl.orders(len(meta["hidden"]))[0][:-2]:
            worst[f"c{it}/{pn}"] = parity.rel_err(gv[pn].cpu().numpy(), want[-1][0][pn].numpy())
        for k in range(it):
            worst[f"c{it}/i{k}/loss"] = parity.rel_err(
                np.array([tr.policy_opt_history["loss"][k]]), np.array([want[k][1]]))
            worst[f"c{it}/i{k}/grad_norm"] = parity.rel_err(
                np.array([tr.policy_opt_history["grad_norm"][k]]), np.array([want[k][2]]))
    print(meta["kind"], meta["hidden"], N, sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    bad = {k: v for k, v in worst.items() if v > 1e-5}
    assert not bad, bad


# N = 37: the small-batch kernels; 1100: the large-batch set, ragged, depth 1;
# 1029 at (13, 6, [80, 80]): test_gpu_ragged's shape for partial tiles
NONE_CASES = [("goac", 1, 1, [16], 2, 37), ("ptrain", 5, 2, [24], 10, 37),
              ("goac", 1, 1, [16], 2, 1100), ("ptrain", 1, 1, [16], 10, 1100),
              ("goac", 13, 6, [80, 80], 2, 1029), ("ptrain", 13, 6, [80, 80], 5, 1029)]


@pytest.mark.parametrize("kind,Do,Da,hidden,K,N", NONE_CASES)
def test_shuffle_none_matches_restatement(kind, Do, Da, hidden, K, N):
    meta = _meta(kind, Do, Da, hidden, K)
    tr = gl.trainer_for(meta)
    _identity_against_restatement(tr, meta, _buffer(Do, Da, N), N)


# ----------------------------------- 4. determinism, buffers and plans
def _sweep_state(tr):
    return (_block(tr, tr.params), _block(tr, tr.adam_m), _block(tr, tr.adam_v),
            list(tr.policy_opt_history["loss"]), list(tr.policy_opt_history["grad_norm"]))


def _same(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("shuffle", ["reference", "none"])
def test_two_runs_are_bitwise_equal(shuffle):
    meta, g = parity.load("ptrain_go_d2")
    out = []
    for _ in range(2):
        tr = gl.trainer_for(meta)
        _train(tr, meta, g, 0)
        random.seed(3)
        tr.optimize_policies(_fixture_buffer(meta), iterations=3, shuffle=shuffle)
        out.append(_sweep_state(tr))
    assert _same(*out)


@pytest.mark.parametrize("shuffle", ["reference", "none"])
def test_device_buffer_and_numpy_dataset_agree_bitwise(shuffle):
    meta, g = parity.load("goac_go_d1")
    out = []
    for buf in (_fixture_buffer(meta), gl.NumpyDataset(gl.dataset_of(meta)),
                _fixture_buffer(meta, capacity=meta["n_replay"])):   # (full: no spare row)
        tr = gl.trainer_for(meta)
        random.seed(3)
        tr.optimize_policies(buf, iterations=3, shuffle=shuffle)
        out.append(_sweep_state(tr))
    assert _same(out[0], out[1]) and _same(out[0], out[2])


def test_growing_replay_keeps_one_sweep_plan():
    meta = _meta("goac", 1, 1, [16])
    tr = gl.trainer_for(meta)
    n_plans = len(tr._plans)
    for N in (1100, 1300):
        rb = _buffer(1, 1, N)
        _identity_against_restatement(tr, meta, rb, N, calls=(1,))
        assert len(tr._plans) == n_plans + 1 and tr._sweep[0][0] == N
    random.seed(0)
    tr.optimize_policies(rb, iterations=2)            # the same N and store: the same plan
    assert len(tr._plans) == n_plans + 1


# ------------------------------------------- the riverswim recipes' calls
RECIPES = [(alg, mu, cnt) for alg in ("g-oac", "p-oac")
           for mu, cnt in ((False, False), (True, False), (True, True))]


@pytest.mark.parametrize("alg,mean_update,counts", RECIPES)
def test_riverswim_recipe_calls(alg, mean_update, counts):
    """reproduce_riverswim.sh's six configurations (--share_layers --global_opt,
    one hidden layer of 16; plain, --mean_update, --mean_update --counts) through
    rl_algorithm.py:160-171's calls: random_batch + train per step, then
    optimize_policies(replay_buffer, ...)."""
    import oac_amd
    Do = Da = 1
    torch.manual_seed(0)
    pp = oac_amd.get_policy_producer(Do, Da, [16])
    common = dict(action_space=Space(Da), discount=0.99, policy_lr=1e-3, qf_lr=1e-3,
                  soft_target_tau=5e-3, q_min=0.0, q_max=500.0, share_layers=True,
                  global_opt=True, mean_update=mean_update, counts=counts)
    if alg == "g-oac":
        tr = oac_amd.GaussianTrainer(pp, oac_amd.get_q_producer(Do, Da, [16], output_size=2),
                                     **common)
    else:
        tr = oac_amd.ParticleTrainer(pp, oac_amd.get_q_producer(Do, Da, [16], output_size=10),
                                     n_estimators=10, **common)
    cls = oac_amd.ReplayBufferCount if counts else oac_amd.ReplayBuffer
    rb = cls(1200, Space(Do), Space(Da))
    data = synthetic_transitions(1100, Do, Da, seed=0)
    rb.load_transitions(torch.from_numpy(rb._rows_from(
        data["observations"], data["actions"], data["rewards"], data["next_observations"],
        data["terminals"])))
    pol0 = _block(tr, tr.params)
    for _ in range(3):
        tr.train(rb.random_batch(32))
    torch.cuda.synchronize()
    assert torch.equal(pol0, _block(tr, tr.params)) and "Policy Loss" not in tr.get_diagnostics()
    random.seed(0)
    tr.optimize_policies(rb, '', 0, False, iterations=3)
    h = tr.policy_opt_history
    assert len(h["loss"]) == 3 and np.all(np.isfinite(h["loss"] + h["grad_norm"]))
    assert not torch.equal(pol0, _block(tr, tr.params))
    assert tr.policy_optimizer.state_dict()["state"][0]["step"] == 3
    assert tr.target_policy_optimizer.state_dict()["state"][0]["step"] == 3


# ------------------------------------------------- 5. snapshot and errors
def test_snapshot_round_trip_continues_bitwise():
    meta, g = parity.load("goac_go_d1")
    rb = _fixture_buffer(meta)

    def head(tr):
        _train(tr, meta, g, 0)
        random.seed(5)
        tr.optimize_policies(rb, iterations=2)

    def tail(tr):
        _train(tr, meta, g, 1)
        random.seed(6)
        tr.optimize_policies(rb, iterations=2)
        return _sweep_state(tr) + (tr.params.clone(), tr.adam_m.clone(), tr.adam_v.clone())

    a = gl.trainer_for(meta)
    head(a)
    buf = io.BytesIO()
    torch.save(a.get_snapshot(), buf)
    assert "init_policy" not in " ".join(a.get_snapshot())
    want = tail(a)
    b = gl.trainer_for(meta)
    buf.seek(0)
    b.restore_from_snapshot(torch.load(buf, weights_only=False))
    assert b._policy_opt_steps == 2 and int(b._popt_state[0].item()) == 2
    assert b.policy_optimizer.state_dict()["state"][0]["step"] == 2
    assert b.target_policy_optimizer.state_dict()["state"][0]["step"] == 1
    assert _same(want, tail(b))
    assert a.init_policy not in a.networks and a.init_target_policy not in a.networks


def test_construction_and_call_errors():
    import oac_amd
    from oac_amd import dp
    meta, _ = parity.load("goac_go_d1")
    with pytest.raises(NotImplementedError, match="ensemble"):
        gl.trainer_for(meta, ensemble=True)
    pmeta, _ = parity.load("ptrain_go_d2")
    pp, qp = gl.producers(pmeta)
    with pytest.raises(NotImplementedError, match="global_opt"):
        oac_amd.ParticleTrainerOAC(pp, qp, n_estimators=10, action_space=Space(2),
                                   share_layers=True, global_opt=True)
    for cls in (dp.DataParallelGaussianTrainer, dp.DataParallelParticleTrainer):
        with pytest.raises(NotImplementedError, match="global_opt"):
            cls(pp, qp, share_layers=True, global_opt=True)
    tr = gl.trainer_for(meta)
    rb = _fixture_buffer(meta)
    with pytest.raises(NotImplementedError, match="policy_opt_history"):
        tr.optimize_policies(rb, save_fig=True)
    with pytest.raises(ValueError, match="shuffle"):
        tr.optimize_policies(rb, shuffle="permute")
    with pytest.raises(RuntimeError, match="global_opt"):
        gl.trainer_for(meta, global_opt=False).optimize_policies(rb)
    assert tr.optimize_policies(rb, iterations=1) is None
    # the C ABI: a global_opt handle takes no graph, phase or all-reduce hook
    from oac_amd import _lib
    L = _lib.lib()
    h = tr._sweep[1].handle
    for call, word in ((lambda: L.oac_sac_step(h, _lib.OAC_STEP_USE_GRAPH, None), "OAC_STEP_USE_GRAPH"),
                       (lambda: L.oac_sac_step_phase(h, 0, 0, None), "oac_sac_step_phase"),
                       (lambda: L.oac_sac_set_allreduce(h, None, None, 0), "oac_sac_set_allreduce")):
        assert call() != 0 and word in L.oac_last_error().decode()
    with pytest.raises(NotImplementedError, match="use_graph"):
        gl.trainer_for(meta, use_graph=True)
