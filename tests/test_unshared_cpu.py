"""CPU checks of share_layers=False (separate critics) for the g-oac and p-oac
trainers: the CPU oracle (tests/unshared_oracle.py) against the reference's own
unshared runs (tests/golden/*_us_*.npz, make_golden_unshared.py), the fixtures'
seed conditions, and the C-ABI boundary -- ``unshared`` / ``std_lr`` in
oac_sac_config, the stacked critic layout, the configurations it rejects."""
import ctypes

import numpy as np
import pytest
import torch

import parity
import test_oracle_golden as tog
import unshared_oracle as uo


# ------------------------------------------------------------------ oracle
_RUNS = {}


def _run(name):
    """(meta, golden, fp32 errors, float64 errors, extras), computed once."""
    if name not in _RUNS:
        meta, g = parity.load(name)
        extras = {}
        errs = uo.oracle_errors(meta, g, extras=extras)
        _RUNS[name] = (meta, g, errs, uo.oracle_errors(meta, g, torch.float64), extras)
    return _RUNS[name]


@pytest.mark.parametrize("name", uo.FIXTURES)
def test_oracle_matches_reference_golden_unshared(name):
    """Every critic's gradient, post-step parameters, target and Adam moments,
    both policies and the statistics of every step under the project's gate
    (max(1e-5, 3x the reference's own fp32 distance from the float64 oracle),
    per key); nothing sampled, nothing left out."""
    meta, g, errs, noise, _ = _run(name)
    assert meta["share_layers"] is False and len(meta["hidden"]) == 1 and meta["steps"] == 3
    K = uo.n_critics(meta)
    for s in range(3):
        for k in range(K):
            for pn in uo.Q_ORDER:
                for what in ("grad", "post", "adam_m", "adam_v"):
                    assert f"s{s}/{what}/qf{k}/{pn}" in errs and f"s{s}/{what}/qf{k}/{pn}" in g
                assert f"s{s}/post/tf{k}/{pn}" in errs
    assert not [k for k in g if "#" in k]          # (no sampled tensor)
    bad = tog.gated(errs, noise)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


@pytest.mark.parametrize("name", [n for n in uo.FIXTURES if n.startswith("ptrain")])
def test_particle_fixtures_rank_margin(name):
    """Seed condition (b): adjacent sorted particle values of every row of
    every step (critics, targets, post-step critics) at least 1e-4 of the
    row's spread apart -- two correct fp32 sums rank every row alike."""
    meta, _, _, _, extras = _run(name)
    assert extras["min_gap"] >= 1e-4
    assert meta["min_gap"] == pytest.approx(extras["min_gap"], rel=1e-3)


def test_crossed_fixture_exercises_the_rank_indicator():
    meta, g, _, _, extras = _run("ptrain_us_crossed")
    assert extras["out_of_rank"] >= 0.10
    # ... and a critic's gradient is not what the full sort backward would give:
    # the "QF Unordered" count the reference recorded is that many pairs
    assert float(g["s0/stat/QF Unordered"]) == round(extras["out_of_rank"] * meta["B"] * meta["K"])
    plain = _run("ptrain_us_plain")
    assert plain[4]["out_of_rank"] == 0.0


def test_fixture_shapes():
    """The riverswim recipes' shape for the six recipe fixtures, the lqg line's
    width 8 (stacked 80), two ragged (5, 2, [24], 37) ones with a frozen bias
    (stacked 48 / 72: 72 is no multiple of 16)."""
    recipe = ["goac_us_plain", "goac_us_counts", "goac_us_mean", "ptrain_us_plain",
              "ptrain_us_counts", "ptrain_us_mean"]
    for name in recipe:
        meta, _ = parity.load(name)
        assert (meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["B"]) == (1, 1, [16], 32)
        assert meta["K"] == (2 if meta["kind"] == "goac" else 10)
    assert parity.load("goac_us_counts")[0]["counts"] and parity.load("ptrain_us_mean")[0]["mean_update"]
    meta, _ = parity.load("ptrain_us_lqg")
    assert (meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["B"], meta["K"]) == (1, 1, [8], 32, 10)
    meta, _ = parity.load("goac_us_nobias")
    assert (meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["B"]) == (5, 2, [24], 37)
    assert meta["train_bias"] is False and meta["std_lr"] != meta["lr"]
    meta, g = parity.load("ptrain_us_nobias_tpn")
    assert (meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["B"], meta["K"]) == (5, 2, [24], 37, 3)
    assert meta["train_bias"] is False and meta["use_target_policy"] is True
    assert (meta["K"] * 24) % 16 != 0 and not g["s0/grad/qf1/last_fc.bias"].any()


def test_frozen_bias_is_the_std_critics_alone_for_g_oac():
    meta, g = parity.load("goac_us_nobias")
    assert g["s0/grad/qf0/last_fc.bias"].any() and not g["s0/grad/qf1/last_fc.bias"].any()
    p = uo.params_of(meta)
    assert np.array_equal(g["s2/post/qf1/last_fc.bias"], p["qfs"][1]["last_fc.bias"])
    assert not np.array_equal(g["s2/post/qf0/last_fc.bias"], p["qfs"][0]["last_fc.bias"])


# ------------------------------------------------------------------ C ABI
GAUSS, PARTICLE_UB = 2, 3
NAMES = {0: b"SAC", 1: b"PARTICLE", 2: b"GAUSS", 3: b"PARTICLE_UB", 4: b"DDPG"}


def _cfg(kind, Do, Da, H, q_out, n_hidden=1, batch=32, **kw):
    from oac_amd import _lib, row_layout
    cfg = _lib.SacConfig()
    cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = (
        kind, Do, Da, H, q_out, batch)
    for k, v in row_layout(Do, Da).items():
        setattr(cfg, k, v)
    cfg.gemm_cfg = -1
    cfg.world_size = 1
    cfg.n_hidden = n_hidden
    cfg.std_lr = 3e-5
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _query(cfg):
    from oac_amd import _lib
    lay = _lib.SacLayout()
    rc = _lib.lib().oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay))
    return rc, lay, _lib.lib().oac_last_error()


def _fields(lay):
    return {n: getattr(lay, n) for n, _ in lay._fields_}


def test_config_fields_and_abi_version():
    from oac_amd import _lib
    assert _lib.lib().oac_abi_version() == 3
    # the C struct: unshared and std_lr are its last fields, after global_opt ...
    names = [n for n, _ in _lib._SacConfigC._fields_]
    assert names[-3:] == ["global_opt", "unshared", "std_lr"]
    # ... and every SacConfig carries the whole struct, the tail zeroed
    c = _lib.SacConfig()
    assert c.unshared == 0 and c.std_lr == 0.0
    assert len(c._buf) == ctypes.sizeof(_lib._SacConfigC) > ctypes.sizeof(_lib.SacConfig)
    tail = _lib._SacConfigC.from_buffer(c._buf)
    c.unshared, c.std_lr, c.global_opt = 1, 3e-5, 1
    assert (tail.unshared, tail.std_lr, tail.global_opt) == (1, 3e-5, 1)
    assert ctypes.addressof(tail) == ctypes.addressof(c)


@pytest.mark.parametrize("kind,K", [(GAUSS, 2), (PARTICLE_UB, 2), (PARTICLE_UB, 3), (PARTICLE_UB, 10),
                                    (PARTICLE_UB, 16)])
@pytest.mark.parametrize("dims", [(1, 1, 16), (1, 1, 8), (5, 2, 24), (7, 5, 52)])
@pytest.mark.parametrize("batch", [32, 1100])
def test_stacked_layout(kind, K, dims, batch):
    """The layout contract of include/oac_amd.h: one critic block of the K
    critics' tensors stacked, critic k = slice k of each, contiguous."""
    Do, Da, H = dims
    Dq = Do + Da
    rc, lay, err = _query(_cfg(kind, Do, Da, H, K, unshared=1, batch=batch))
    assert rc == 0, err
    al4 = lambda n: (n + 3) // 4 * 4
    assert lay.n_critics == K and lay.q2_base == -1
    assert lay.q_fc1_w == -1 and lay.q_fc1_b == -1 and lay.pol_fc1_w == -1
    # stacked tensors [K H, Dq], [K H], [K H], [K]: in order, nothing between them
    assert (lay.q_fc0_w, lay.q_fc0_b) == (0, K * H * Dq)
    assert lay.q_last_w == lay.q_fc0_b + K * H
    assert lay.q_last_b == lay.q_last_w + K * H
    assert lay.q_size == lay.q_last_b + al4(K)
    # critic k's slices: contiguous, the first three 16-byte aligned
    for k in range(K):
        for off, n in ((lay.q_fc0_w + k * H * Dq, H * Dq), (lay.q_fc0_b + k * H, H),
                       (lay.q_last_w + k * H, H)):
            assert off % 4 == 0 and n % 4 == 0
        assert lay.q_last_b + k < lay.q_size
    assert (lay.tpol_base, lay.q1_base) == (lay.pol_size, 2 * lay.pol_size)
    assert lay.params_total == 2 * lay.pol_size + lay.q_size
    assert lay.targets_total == lay.q_size and lay.workspace_floats > 0
    # against the shared layout of the same dimensions: the policy blocks are
    # the same; the critic block holds K H (Dq + 1) + K H + K instead of
    # H (Dq + 1) + K H + K floats
    rc, sh, err = _query(_cfg(kind, Do, Da, H, K, unshared=0, batch=batch))
    assert rc == 0, err
    for f in ("pol_fc0_w", "pol_fc0_b", "pol_head_w", "pol_head_b", "pol_size", "tpol_base",
              "q1_base"):
        assert getattr(sh, f) == getattr(lay, f), f
    assert sh.n_critics == 1 and sh.q_last_b - sh.q_last_w == al4(K * H)
    assert lay.q_size - sh.q_size == (K - 1) * H * (Dq + 1)


@pytest.mark.parametrize("kind,q_out,n_hidden", [(0, 1, 2), (1, 5, 2), (GAUSS, 2, 1), (GAUSS, 2, 2),
                                                 (PARTICLE_UB, 10, 1), (PARTICLE_UB, 10, 0),
                                                 (4, 1, 2)])
def test_zero_and_unset_configs_keep_their_layouts(kind, q_out, n_hidden):
    """unshared = 0 (a zero-initialised tail) is the layout of a config without
    the fields, whatever std_lr holds."""
    base = _cfg(kind, 11, 3, 32, q_out, n_hidden)
    base.std_lr = 0.0
    rc0, a, err = _query(base)
    assert rc0 == 0, err
    rc1, b, err = _query(_cfg(kind, 11, 3, 32, q_out, n_hidden, unshared=0, std_lr=123.0))
    assert rc1 == 0, err
    assert _fields(a) == _fields(b)
    assert a.n_critics == (2 if kind == 0 else 1)
    H, Dq = 32, 14
    two = n_hidden != 1
    assert a.q_size == H * Dq + H + (H * H + H if two else 0) + (q_out * H + 3) // 4 * 4 + \
        (q_out + 3) // 4 * 4


REJECTED = [
    # (config overrides, the field the message must name)
    (dict(kind=0, q_out=1, n_hidden=2), b"unshared"),
    (dict(kind=1, q_out=5, n_hidden=2), b"unshared"),
    (dict(kind=4, q_out=1, n_hidden=2), b"unshared"),
    (dict(kind=GAUSS, q_out=2, n_hidden=2), b"n_hidden"),
    (dict(kind=GAUSS, q_out=2, n_hidden=0), b"n_hidden"),
    (dict(kind=PARTICLE_UB, q_out=10, n_hidden=2), b"n_hidden"),
    (dict(kind=GAUSS, q_out=2, world_size=2), b"world_size"),
    (dict(kind=PARTICLE_UB, q_out=10, world_size=2), b"world_size"),
    (dict(kind=GAUSS, q_out=2, global_opt=1), b"global_opt"),
    (dict(kind=PARTICLE_UB, q_out=10, global_opt=1), b"global_opt"),
    (dict(kind=GAUSS, q_out=2, hidden=18), b"hidden"),
    (dict(kind=PARTICLE_UB, q_out=10, hidden=18), b"hidden"),
    (dict(kind=GAUSS, q_out=2, std_lr=0.0), b"std_lr"),
    (dict(kind=GAUSS, q_out=2, unshared=2), b"unshared"),
]


@pytest.mark.parametrize("over,field", REJECTED)
def test_rejected_configurations_name_field_and_kind(over, field):
    """oac_sac_query_layout and oac_sac_create reject the same configs, and the
    message names the offending field and the kind."""
    from oac_amd import _lib
    L = _lib.lib()
    kw = dict(kind=GAUSS, Do=3, Da=2, H=16, q_out=2, unshared=1)
    kw.update(over)
    H = kw.pop("hidden", kw.pop("H"))
    cfg = _cfg(kw.pop("kind"), kw.pop("Do"), kw.pop("Da"), H, kw.pop("q_out"), **kw)
    rc, _, msg = _query(cfg)
    assert rc != 0
    assert field in msg and (b"kind %d" % cfg.kind) in msg, msg
    if cfg.unshared == 1:
        assert NAMES[cfg.kind] in msg, msg
    bufs = _lib.SacBuffers()
    h = ctypes.c_void_p()
    assert L.oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h)) != 0
    msg2 = L.oac_last_error()
    assert field in msg2 and (b"kind %d" % cfg.kind) in msg2 and not h.value


@pytest.mark.parametrize("kind,q_out", [(GAUSS, 1), (GAUSS, 3), (PARTICLE_UB, 1), (PARTICLE_UB, 17)])
def test_the_number_of_critics_is_bounded(kind, q_out):
    rc, _, msg = _query(_cfg(kind, 3, 2, 16, q_out, unshared=1))
    assert rc != 0 and b"q_out" in msg, msg
