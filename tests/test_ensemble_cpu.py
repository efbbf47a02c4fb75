"""The policy ensemble (ParticleTrainer ensemble=True) without a GPU: the CPU
oracle (tests/ensemble_oracle.py) against the reference's own runs
(tests/golden/ens_*.npz), the fixtures' seed conditions re-measured, the C
ABI's layout contract and rejections (oac_sac_query_layout_ensemble /
oac_sac_create_ensemble: host-only calls), the producers' biases and the
margins of the GPU sweep's cases."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import parity
import test_oracle_golden as tog
from test_unshared_cpu import _cfg, _fields, _query

PARTICLE_UB, GAUSS = 3, 2


# ----------------------------------------------------------------- fixtures
_RUNS = {}


def _run(name):
    """One fp32 and one float64 oracle run per fixture, shared by the tests."""
    if name not in _RUNS:
        meta, g = parity.load(name)
        extras = {}
        errs = eo.oracle_errors(meta, g, extras=extras)
        noise = eo.oracle_errors(meta, g, torch.float64)
        _RUNS[name] = (meta, g, errs, noise, extras)
    return _RUNS[name]


@pytest.mark.parametrize("name", eo.FIXTURES)
def test_oracle_matches_reference_golden(name):
    """Every recorded tensor of every step, whole (no sampled tensor), under
    the project's gate; oracle_errors asserts the chosen indices equal."""
    meta, g, errs, noise, _ = _run(name)
    assert not [k for k in g if "#" in k]
    assert set(errs) == set(noise) and len(errs) > 100
    bad = tog.gated(errs, noise)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


@pytest.mark.parametrize("name", eo.FIXTURES)
def test_seed_conditions_hold_and_equal_meta(name):
    meta, g, _, _, extras = _run(name)
    assert extras["min_gap"] == meta["min_gap"] >= eo.MIN_GAP                       # (b)
    if meta["mean_update"]:
        assert "s0/sel" not in g and extras["sel_gap"] == float("inf")
    else:
        assert extras["sel_gap"] == meta["sel_gap"] >= eo.MIN_GAP                   # (c)
        assert extras["chosen_share"] == meta["chosen_share"]
    if name == "ens_plain":                                                         # (d)
        assert sum(v >= 0.10 for v in meta["chosen_share"]) >= 2


def test_fixture_shapes_and_the_initial_action_quirk():
    for name in ("ens_plain", "ens_counts", "ens_mean"):
        m, _ = parity.load(name)
        assert (m["obs_dim"], m["act_dim"], m["hidden"], m["B"], m["K"], m["P"]) == (2, 1, [16], 32, 10, 5)
        want = np.linspace(-1., 1., 5)
        want[0] += 5e-2
        want[-1] -= 5e-2
        assert m["initial_actions"] == want.tolist()
    assert parity.load("ens_counts")[0]["counts"] and parity.load("ens_mean")[0]["mean_update"]
    m, g = parity.load("ens_ragged")
    assert (m["obs_dim"], m["act_dim"], m["hidden"], m["B"], m["K"], m["P"]) == (5, 3, [24], 37, 3, 3)
    assert m["train_bias"] is False and not g["s0/grad/qf1/last_fc.bias"].any()
    # act_dim > 1: P * Da draws on numpy's global stream, the first P of them used
    draws = np.random.RandomState(m["np_seed"]).uniform(-1, 1, (3, 3)).astype(np.float32).flatten()
    assert len(m["initial_actions"]) == 9
    assert np.allclose(m["initial_actions"], draws, rtol=1e-6)
    p = eo.params_of(m)
    for i in range(3):
        assert np.array_equal(p["policies"][i]["last_fc.bias"],
                              np.full(3, np.arctanh(m["initial_actions"][i]), np.float32))
    assert g["act/obs"].shape == (64, 5) and g["act/forward/action"].shape == (64, 3)


def test_acting_oracle_matches_the_recorded_observations():
    m, g = parity.load("ens_ragged")
    s = m["steps"] - 1
    base = eo.params_of(m)
    params = dict(policies=[{pn: g[f"s{s}/post/policy{p}/{pn}"] for pn in eo.POL_ORDER}
                            for p in range(m["P"])],
                  qfs=[{pn: g[f"s{s}/post/qf{k}/{pn}"] for pn in eo.Q_ORDER} for k in range(m["K"])],
                  tfs=base["tfs"], target_policy=base["target_policy"])
    params["policy"] = params["policies"][0]
    act = eo.make_oracle(m, params=params).act(g["act/obs"])
    assert np.array_equal(act["sel"].numpy(), g["act/sel"])
    assert act["sel_gap"] == m["act_sel_gap"] >= eo.MIN_GAP
    assert len(set(g["act/sel"].tolist())) >= 2
    assert parity.rel_err(act["proposals"].numpy(), g["act/proposals"]) < 1e-5
    assert parity.rel_err(act["ub"].numpy(), g["act/ub"]) < 1e-5
    # (get_action ran one row at a time, forward all 64 at once)
    assert parity.rel_err(g["act/get_action"], g["act/forward/action"]) < 1e-6
    for nm in ("action", "mean", "log_std", "log_prob", "std", "pre_tanh"):
        assert parity.rel_err(act[nm].numpy(), g[f"act/forward/{nm}"]) < 1e-5, nm


# -------------------------------------------------------------------- C ABI
def _query_ens(cfg, P):
    from oac_amd import _lib
    lay, ens = _lib.SacLayout(), _lib.EnsembleLayout()
    rc = _lib.lib().oac_sac_query_layout_ensemble(ctypes.byref(cfg), P, ctypes.byref(lay),
                                                  ctypes.byref(ens))
    return rc, lay, ens, _lib.lib().oac_last_error()


@pytest.mark.parametrize("P", [1, 2, 5, 16])
@pytest.mark.parametrize("dims", [(1, 1, 16), (1, 1, 8), (5, 2, 24), (7, 5, 52)])
@pytest.mark.parametrize("batch", [32, 1100])
def test_stacked_policy_layout(P, dims, batch):
    """include/oac_amd.h: one policy block of the P policies' tensors stacked,
    policy p = slice p of each, contiguous; then the single-policy
    target_policy block, then the critic block; everything else as the plain
    unshared layout."""
    Do, Da, H = dims
    K = 3
    cfg = _cfg(PARTICLE_UB, Do, Da, H, K, unshared=1, batch=batch)
    rc, lay, ens, err = _query_ens(cfg, P)
    assert rc == 0, err
    al4 = lambda n: (n + 3) // 4 * 4
    assert ens.n_policies == P
    assert (ens.ens_fc0_w, ens.ens_fc0_b) == (0, P * H * Do)
    assert ens.ens_head_w == ens.ens_fc0_b + P * H
    assert ens.ens_head_b == ens.ens_head_w + P * 2 * Da * H
    assert ens.ens_size == ens.ens_head_b + al4(P * 2 * Da)
    for p in range(P):   # policy p's slices: the first three 16-byte aligned
        for off, n in ((ens.ens_fc0_w + p * H * Do, H * Do), (ens.ens_fc0_b + p * H, H),
                       (ens.ens_head_w + p * 2 * Da * H, 2 * Da * H)):
            assert off % 4 == 0 and n % 4 == 0
        assert ens.ens_head_b + (p + 1) * 2 * Da <= ens.ens_size
    rc, plain, err = _query(cfg)
    assert rc == 0, err
    # the target_policy block keeps a single policy's shape
    for f in ("fc0_w", "fc0_b", "head_w", "head_b", "size"):
        assert getattr(ens, "tpol_" + f) == getattr(plain, "pol_" + f) == getattr(lay, "pol_" + f)
    assert lay.tpol_base == ens.ens_size and lay.q1_base == ens.ens_size + lay.pol_size
    assert lay.params_total == lay.q1_base + lay.q_size
    moved = {"tpol_base", "q1_base", "params_total", "workspace_floats"}
    assert {k: v for k, v in _fields(lay).items() if k not in moved} == \
        {k: v for k, v in _fields(plain).items() if k not in moved}
    assert lay.workspace_floats > plain.workspace_floats


@pytest.mark.parametrize("kind,q_out,n_hidden,unshared", [
    (0, 1, 2, 0), (1, 5, 2, 0), (GAUSS, 2, 1, 1), (PARTICLE_UB, 10, 1, 1), (PARTICLE_UB, 10, 2, 0),
    (4, 1, 2, 0)])
def test_zero_policies_is_the_plain_query(kind, q_out, n_hidden, unshared):
    cfg = _cfg(kind, 11, 3, 32, q_out, n_hidden, unshared=unshared)
    rc0, a, err = _query(cfg)
    assert rc0 == 0, err
    rc1, b, ens, err = _query_ens(cfg, 0)
    assert rc1 == 0, err
    assert _fields(a) == _fields(b)
    assert not any(_fields(ens).values())


ENS_REJECTED = [
    # (config overrides, n_policies, the field the message must name)
    (dict(kind=0, q_out=1, n_hidden=2, unshared=0), 5, b"kind"),
    (dict(kind=GAUSS, q_out=2), 5, b"kind"),
    (dict(unshared=0), 5, b"unshared"),
    (dict(n_hidden=2), 5, b"n_hidden"),
    (dict(n_hidden=0), 5, b"n_hidden"),
    (dict(world_size=2), 5, b"world_size"),
    (dict(global_opt=1), 5, b"global_opt"),
    (dict(hidden=18), 5, b"hidden"),
    (dict(), 17, b"n_policies"),
    (dict(), -1, b"n_policies"),
]


@pytest.mark.parametrize("over,P,field", ENS_REJECTED)
def test_rejected_ensemble_configurations_name_field_and_kind(over, P, field):
    from oac_amd import _lib
    L = _lib.lib()
    kw = dict(kind=PARTICLE_UB, Do=3, Da=2, H=16, q_out=10, unshared=1)
    kw.update(over)
    H = kw.pop("hidden", kw.pop("H"))
    cfg = _cfg(kw.pop("kind"), kw.pop("Do"), kw.pop("Da"), H, kw.pop("q_out"), **kw)
    rc, _, _, msg = _query_ens(cfg, P)
    assert rc != 0
    assert b"ensemble" in msg and field in msg and (b"kind %d" % cfg.kind) in msg, msg
    h = ctypes.c_void_p()
    bufs = _lib.SacBuffers()
    assert L.oac_sac_create_ensemble(ctypes.byref(cfg), P, ctypes.byref(bufs), ctypes.byref(h)) != 0
    msg2 = L.oac_last_error()
    assert b"ensemble" in msg2 and field in msg2 and (b"kind %d" % cfg.kind) in msg2 and not h.value


def test_create_rejects_a_next_policy_block_and_the_handle_its_calls():
    """Host-only: with null buffers create makes no GPU call, and the three
    rejected calls return before any launch."""
    from oac_amd import _lib
    L = _lib.lib()
    cfg = _cfg(PARTICLE_UB, 2, 1, 16, 10, unshared=1)
    h, bufs = ctypes.c_void_p(), _lib.SacBuffers()
    dummy = (ctypes.c_float * 4)()
    bufs.next_policy = ctypes.cast(dummy, ctypes.c_void_p)
    assert L.oac_sac_create_ensemble(ctypes.byref(cfg), 5, ctypes.byref(bufs), ctypes.byref(h)) != 0
    msg = L.oac_last_error()
    assert b"ensemble" in msg and b"next_policy" in msg and b"PARTICLE_UB" in msg and not h.value
    bufs = _lib.SacBuffers()
    assert L.oac_sac_create_ensemble(ctypes.byref(cfg), 5, ctypes.byref(bufs), ctypes.byref(h)) == 0
    try:
        assert L.oac_sac_step(h, _lib.OAC_STEP_USE_GRAPH, None) != 0
        assert b"ensemble" in L.oac_last_error() and b"OAC_STEP_USE_GRAPH" in L.oac_last_error()
        assert L.oac_sac_step_phase(h, 0, 0, None) != 0
        assert b"ensemble" in L.oac_last_error() and b"oac_sac_step_phase" in L.oac_last_error()
        assert L.oac_sac_set_allreduce(h, None, None, 0) != 0
        assert b"ensemble" in L.oac_last_error() and b"oac_sac_set_allreduce" in L.oac_last_error()
        off, rows, cols = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        lay, ens = _lib.SacLayout(), _lib.EnsembleLayout()
        assert L.oac_sac_query_layout_ensemble(ctypes.byref(cfg), 5, ctypes.byref(lay),
                                               ctypes.byref(ens)) == 0
        shapes = {}
        for name, which in _lib.ENS_VIEWS.items():
            assert L.oac_sac_ensemble_view(h, which, ctypes.byref(off), ctypes.byref(rows),
                                           ctypes.byref(cols)) == 0, name
            assert off.value + rows.value * cols.value <= lay.workspace_floats
            shapes[name] = (rows.value, cols.value)
        assert shapes == dict(sel=(32, 1), ub_next=(32, 5), act=(32, 5), head=(32, 10),
                              ub_obs=(32, 5))
        assert L.oac_sac_ensemble_view(h, len(_lib.ENS_VIEWS), ctypes.byref(off), ctypes.byref(rows),
                                       ctypes.byref(cols)) != 0
    finally:
        assert L.oac_sac_destroy(h) == 0
    # a plain handle has no ensemble views
    assert L.oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h)) == 0
    try:
        assert L.oac_sac_ensemble_view(h, 0, ctypes.byref(off), ctypes.byref(rows),
                                       ctypes.byref(cols)) != 0
        assert b"oac_sac_create_ensemble" in L.oac_last_error()
    finally:
        assert L.oac_sac_destroy(h) == 0


def test_ensemble_eval_rejects_bad_arguments_by_name():
    """oac_ensemble_eval checks its dimensions before any launch (host-only)."""
    from oac_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    offs = (ctypes.c_int64 * 4)(0, 0, 0, 0)

    def call(P=5, K=10, di=8, Do=2, Da=1, H=16, n=0):
        return L.oac_ensemble_eval(p, offs, P, p, offs, K, di, Do, Da, H, p, Do, n, None, p, p, p,
                                   p, p, None, p, p, None)
    assert call() == 0, L.oac_last_error()   # n = 0: no launch
    for kw, word in ((dict(P=0), b"n_policies"), (dict(P=17), b"n_policies"),
                     (dict(K=17), b"n_critics"), (dict(di=10), b"delta_index"),
                     (dict(Da=33), b"act_dim"), (dict(H=4096, n=1), b"LDS")):
        assert call(**kw) != 0, kw
        assert b"ensemble eval" in L.oac_last_error() and word in L.oac_last_error(), kw


# ---------------------------------------------------------------- producers
def test_policy_producer_honours_ensemble():
    """get_policy_producer(...)(ensemble=True): an object with .policies, policy
    i's mean-head bias arctanh(bias[i]) in every action dimension -- for
    act_dim > 1 only the first n_policies entries of ``bias`` are used."""
    from oac_amd.producers import get_policy_producer
    pp = get_policy_producer(5, 3, [24], device="cpu")
    bias = np.random.RandomState(0).uniform(-1, 1, (4, 3)).flatten()
    ens = pp(bias=bias, ensemble=True, n_policies=4, approximator="me", share_layers=False)
    assert len(ens.policies) == ens.n_policies == 4 and ens.approximator == "me"
    assert ens.share_layers is False
    for i, pol in enumerate(ens.policies):
        sd = pol.state_dict()
        assert list(sd) == eo.POL_ORDER
        assert torch.equal(sd["last_fc.bias"],
                           torch.full((3,), float(np.float32(np.arctanh(bias[i])))))
        assert sd["fc0.weight"].shape == (24, 5) and sd["last_fc_log_std.weight"].shape == (3, 24)
    assert len(ens.state_dict()) == 4
    assert not torch.equal(ens.policies[0].fc0.weight, ens.policies[1].fc0.weight)
    plain = pp()   # (the plain call is what it was)
    assert list(plain.state_dict()) == eo.POL_ORDER and abs(float(plain.last_fc.bias.detach()[0])) <= 1e-3
    with pytest.raises(NotImplementedError, match="share_layers"):
        pp(bias=bias, ensemble=True, n_policies=4, share_layers=True)


# ------------------------------------------------------------- sweep margins
@pytest.mark.parametrize("name", sorted(eo.SWEEP))
def test_sweep_case_margins(name):
    """The GPU sweep compares every row: at its committed seed each case keeps
    adjacent sorted particles and the two best proposals >= 1e-4 of the row's
    spread apart in the compared step (float32 and float64 agree on that)."""
    meta, B = eo.SWEEP[name]
    for dtype in (torch.float32, torch.float64):
        gap, sel_gap = eo.sweep_margins(meta, B, dtype)
        assert gap >= eo.MIN_GAP and sel_gap >= eo.MIN_GAP, (name, dtype, gap, sel_gap)
