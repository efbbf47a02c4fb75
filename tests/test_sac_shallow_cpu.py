"""CPU checks of the one-hidden-layer SAC / OAC support (OAC_KIND_SAC_SHALLOW,
``oac_amd.ShallowSACTrainer``): the CPU oracle against the reference's own
depth-1 runs (tests/golden/sac_d1_*.npz, oac_expl_d1_*.npz;
make_golden_sac_shallow.py), and the C-ABI boundary -- the kind-5 layout, what
the kind refuses (by name), and what keeps being refused for kind 0."""
import ctypes

import pytest
import torch

import parity
import sac_shallow_lib as ssl
import test_oracle_golden as tog
from oracle import sac_oracle as so

KIND = 5


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("name", ssl.STEP_FIXTURES)
def test_oracle_matches_reference_golden(name):
    """Every gradient, post-step parameter, target, Adam moment (whole, no
    element left out) and statistic of every step under parity.gate."""
    meta, g = parity.load(name)
    assert len(meta["hidden"]) == 1 and "s0/grad/qf1/fc1.weight" not in g
    errs = ssl.oracle_errors(meta, g)
    noise = ssl.oracle_noise(meta, g)
    bad = tog.gated(errs, noise)
    print(name, "worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


def test_fixture_shapes():
    want = {"sac_d1_riverswim": (1, 1, [16], 32, 3, True, 1),
            "sac_d1_lqg": (1, 1, [8], 32, 3, True, 1),
            "sac_d1_noalpha_period2": (5, 2, [24], 37, 3, False, 2),
            "sac_d1_mid": (5, 2, [24], 37, 1, True, 1)}
    assert sorted(want) == sorted(ssl.STEP_FIXTURES)
    for name, w in want.items():
        meta, g = parity.load(name)
        assert (meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["B"], meta["steps"],
                meta["auto_alpha"], meta["target_update_period"]) == w
        assert (meta["pi_init_w"], meta["q_init_w"]) == (0.2, 0.1)
        for grp in ssl.GROUPS:   # whole tensors, Adam moments included
            assert f"s0/grad/{grp}/fc0.weight" in g and f"s0/adam/{grp}/fc0.weight/exp_avg_sq" in g
    assert parity.load("sac_d1_mid")[0]["mid_state"]["t"] == 7


@pytest.mark.parametrize("name", ssl.EXPL_FIXTURES)
def test_exploration_oracle_matches_reference_golden(name):
    meta, g = parity.load(name)
    assert len(meta["hidden"]) == 1 and meta["n_obs"] == 16
    assert (meta["beta_UB"], meta["delta"]) == (4.66, 23.53)
    P, Q1, Q2 = (so.to_torch_params(ssl.params_of(meta)[k]) for k in ("policy", "qf1", "qf2"))
    for i in range(meta["n_obs"]):
        r = so.oac_exploration_action(g["obs"][i], P, Q1, Q2, meta["beta_UB"], meta["delta"],
                                      g["eps_discard"][i], g["eps"][i])
        assert parity.rel_err(r["std"].numpy(), g["std"][i]) <= 1e-6
        assert parity.rel_err(r["mu_E"].numpy(), g["mu_E"][i]) <= parity.TOL
        assert parity.rel_err(r["action"].numpy(), g["action"][i]) <= parity.TOL


def test_reference_checkpoint_is_depth_1():
    import os
    fx = torch.load(os.path.join(parity.GOLDEN, "sac_d1_snapshot.pt"), weights_only=True)
    assert fx["meta"]["hidden"] == [16]
    from shallow_lib import orders
    assert list(fx["snapshot"]["policy_state_dict"]) == orders(1)[0]
    assert list(fx["snapshot"]["qf1_state_dict"]) == orders(1)[1]


# ------------------------------------------------------------------ C ABI
def _cfg(kind, Do, Da, H, q_out=1, n_hidden=1, batch=32, **kw):
    from oac_amd import _lib, row_layout
    cfg = _lib.SacConfig()
    cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = (
        kind, Do, Da, H, q_out, batch)
    for k, v in row_layout(Do, Da).items():
        setattr(cfg, k, v)
    cfg.gemm_cfg = -1
    cfg.world_size = 1
    cfg.n_hidden = n_hidden
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _query(cfg):
    from oac_amd import _lib
    L = _lib.lib()
    lay = _lib.SacLayout()
    rc = L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay))
    return rc, lay, L.oac_last_error()


def test_kind_value_and_abi_version():
    from oac_amd import _lib
    assert _lib.OAC_KIND_SAC_SHALLOW == KIND
    assert _lib.lib().oac_abi_version() == 3


@pytest.mark.parametrize("dims", [(1, 1, 16), (1, 1, 8), (5, 2, 24), (7, 5, 52), (376, 17, 256)])
@pytest.mark.parametrize("batch", [1, 32, 600])
def test_kind_5_layout(dims, batch):
    """Kind 0's layout without the fc1 tensors: [policy | critic 1 | critic 2],
    targets = [target critic 1 | target critic 2], no target_policy block."""
    Do, Da, H = dims
    rc, lay, msg = _query(_cfg(KIND, Do, Da, H, batch=batch))
    assert rc == 0, msg
    assert lay.pol_fc1_w == -1 and lay.pol_fc1_b == -1 and lay.q_fc1_w == -1 and lay.q_fc1_b == -1
    al4 = lambda n: (n + 3) // 4 * 4
    assert (lay.pol_fc0_w, lay.pol_fc0_b) == (0, al4(H * Do))
    assert lay.pol_head_w == lay.pol_fc0_b + al4(H)
    assert lay.pol_head_b == lay.pol_head_w + al4(2 * Da * H)
    assert lay.pol_size == lay.pol_head_b + al4(2 * Da)
    assert (lay.q_fc0_w, lay.q_fc0_b) == (0, al4(H * (Do + Da)))
    assert lay.q_last_w == lay.q_fc0_b + al4(H)
    assert lay.q_last_b == lay.q_last_w + al4(H)
    assert lay.q_size == lay.q_last_b + 4
    assert lay.n_critics == 2 and lay.tpol_base == -1
    assert (lay.q1_base, lay.q2_base) == (lay.pol_size, lay.pol_size + lay.q_size)
    assert lay.params_total == lay.pol_size + 2 * lay.q_size and lay.targets_total == 2 * lay.q_size
    assert lay.workspace_floats > 0
    rc, two, msg = _query(_cfg(0, Do, Da, H, n_hidden=2, batch=batch))
    assert rc == 0, msg
    assert two.pol_size == lay.pol_size + al4(H * H) + al4(H)
    assert two.q_size == lay.q_size + al4(H * H) + al4(H)


def test_every_public_view_of_a_kind_5_handle_fits_its_workspace():
    """Host-only: with null buffers create makes no GPU call."""
    from oac_amd import _lib
    L = _lib.lib()
    cfg = _cfg(KIND, 11, 3, 32, batch=40)
    rc, lay, msg = _query(cfg)
    assert rc == 0, msg
    h = ctypes.c_void_p()
    bufs = _lib.SacBuffers()
    assert L.oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h)) == 0, L.oac_last_error()
    try:
        off, rows, cols = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        for name, which in _lib.WS.items():
            assert L.oac_sac_workspace_view(h, which, ctypes.byref(off), ctypes.byref(rows),
                                            ctypes.byref(cols)) == 0, name
            assert off.value + rows.value * cols.value <= lay.workspace_floats, name
        for name, shape in (("batch", (40, cfg.row_stride)), ("eps1", (40, 3)), ("head1", (40, 6)),
                            ("q1", (40, 1)), ("qnew", (40, 1)), ("h1p", (40, 32)), ("h2p", (0, 0))):
            L.oac_sac_workspace_view(h, _lib.WS[name], ctypes.byref(off), ctypes.byref(rows),
                                     ctypes.byref(cols))
            assert (rows.value, cols.value) == shape, name
    finally:
        assert L.oac_sac_destroy(h) == 0


@pytest.mark.parametrize("kw,words", [
    (dict(n_hidden=0), (b"n_hidden", b"OAC_KIND_SAC")),
    (dict(n_hidden=2), (b"n_hidden", b"OAC_KIND_SAC")),
    (dict(n_hidden=3), (b"n_hidden",)),
    (dict(q_out=2), (b"q_out",)),
    (dict(H=18), (b"multiple of 4", b"18")),
    (dict(world_size=2), (b"world_size", b"single-process")),
    (dict(global_opt=1), (b"global_opt",)),
    (dict(unshared=1), (b"unshared",)),
])
def test_kind_5_config_refusals_by_name(kw, words):
    kw = dict(kw)
    H = kw.pop("H", 16)
    q_out = kw.pop("q_out", 1)
    n_hidden = kw.pop("n_hidden", 1)
    cfg = _cfg(KIND, 3, 2, H, q_out=q_out, n_hidden=n_hidden, **kw)
    rc, _, msg = _query(cfg)
    assert rc != 0
    for w in words:
        assert w in msg, (w, msg)
    if b"multiple of 4" not in msg:
        assert b"SAC_SHALLOW" in msg and b"kind 5" in msg, msg
    # oac_sac_create validates the same config before it touches a buffer
    from oac_amd import _lib
    h = ctypes.c_void_p()
    bufs = _lib.SacBuffers()
    assert _lib.lib().oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h)) != 0
    assert not h.value


def test_kind_0_with_one_hidden_layer_is_still_refused_and_points_at_kind_5():
    rc, _, msg = _query(_cfg(0, 11, 3, 32, n_hidden=1))
    assert rc != 0
    for w in (b"n_hidden", b"SAC", b"kind 0", b"GAUSS", b"PARTICLE_UB", b"SAC_SHALLOW", b"kind 5"):
        assert w in msg, (w, msg)


def test_kinds_past_5_stay_rejected():
    for kind in (6, 7, -1):
        rc, _, msg = _query(_cfg(kind, 11, 3, 16))
        assert rc != 0 and b"bad kind" in msg, (kind, msg)


def _handle(cfg):
    from oac_amd import _lib
    h = ctypes.c_void_p()
    bufs = _lib.SacBuffers()
    rc = _lib.lib().oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h))
    return rc, h


def test_large_batch_kernel_set_is_refused_at_create_by_name():
    from oac_amd import _lib
    L = _lib.lib()
    for kw in (dict(batch=1024), dict(batch=4096), dict(batch=32, gemm_cfg=2), dict(batch=32, gemm_cfg=1)):
        cfg = _cfg(KIND, 5, 2, 24, **kw)
        assert _query(cfg)[0] == 0      # (the layout itself exists)
        rc, h = _handle(cfg)
        msg = L.oac_last_error()
        assert rc != 0 and not h.value
        assert b"SAC_SHALLOW" in msg and b"kind 5" in msg and b"large-batch" in msg, msg
    for kw in (dict(batch=1023), dict(batch=2048, gemm_cfg=0)):   # the small kernel set
        rc, h = _handle(_cfg(KIND, 5, 2, 24, **kw))
        assert rc == 0, L.oac_last_error()
        assert L.oac_sac_destroy(h) == 0
    rc, h = _handle(_cfg(KIND, 5, 33, 24))
    assert rc != 0 and b"act_dim <= 32" in L.oac_last_error()


def test_single_process_entry_points_fail_by_name():
    """No data-parallel step and no captured graph for this kind: step_phase,
    set_allreduce, set_step_graph and OAC_STEP_USE_GRAPH fail by name, before
    any launch (host-only)."""
    from oac_amd import _lib
    L = _lib.lib()
    rc, h = _handle(_cfg(KIND, 5, 2, 24))
    assert rc == 0, L.oac_last_error()
    try:
        for call, entry in ((lambda: L.oac_sac_step_phase(h, 0, 0, None), b"oac_sac_step_phase"),
                            (lambda: L.oac_sac_set_allreduce(h, None, None, 0), b"oac_sac_set_allreduce"),
                            (lambda: L.oac_sac_set_step_graph(h, None, 0), b"oac_sac_set_step_graph")):
            assert call() != 0
            msg = L.oac_last_error()
            assert entry in msg and b"SAC_SHALLOW" in msg and b"kind 5" in msg, msg
        for n in (1, 4):
            assert L.oac_sac_step_n(h, _lib.OAC_STEP_USE_GRAPH, n, None) != 0
            msg = L.oac_last_error()
            assert b"OAC_STEP_USE_GRAPH" in msg and b"SAC_SHALLOW" in msg and b"kind 5" in msg, msg
    finally:
        assert L.oac_sac_destroy(h) == 0
