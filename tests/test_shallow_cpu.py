"""CPU checks of the one-hidden-layer (``--num_layers 1``) support: the CPU
oracle against the reference's own depth-1 runs (tests/golden/*_d1_*.npz,
make_golden_shallow.py), and the C-ABI boundary -- ``n_hidden`` in
oac_sac_config, the depth-1 arena layout, the kinds that reject it."""
import ctypes

import pytest
import torch

import parity
import shallow_lib as sl
import test_oracle_golden as tog


@pytest.mark.parametrize("name", sl.FIXTURES)
def test_oracle_matches_reference_golden_at_depth_1(name):
    """Every gradient, post-step parameter and statistic of every step under
    the project's gate (max(1e-5, 3x the reference's own fp32 distance from
    the float64 oracle), per key)."""
    meta, g = parity.load(name)
    assert len(meta["hidden"]) == 1
    errs = sl.oracle_errors(meta, g)
    noise = sl.oracle_errors(meta, g, torch.float64)
    bad = tog.gated(errs, noise)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


def test_fixture_shapes():
    """The recipe shape (riverswim: obs 1, act 1, hidden 16, batch 32) for the
    six recipe fixtures, K = 10 particles; (5, 2, 24, 37) for the seventh."""
    for name in sl.FIXTURES[:6]:
        meta, g = parity.load(name)
        assert (meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["B"], meta["steps"]) == \
            (1, 1, [16], 32, 3)
        assert meta["K"] == (2 if meta["kind"] == "goac" else 10)
        assert "s0/grad/qf/fc1.weight" not in g and "s0/grad/qf/fc0.weight" in g
    meta, _ = parity.load(sl.FIXTURES[6])
    assert (meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["B"]) == (5, 2, [24], 37)
    assert meta["train_bias"] is False and meta["use_target_policy"] is True


# ------------------------------------------------------------------ C ABI
def _cfg(kind, Do, Da, H, q_out, n_hidden, batch=32):
    from oac_amd import _lib, row_layout
    cfg = _lib.SacConfig()
    cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = (
        kind, Do, Da, H, q_out, batch)
    for k, v in row_layout(Do, Da).items():
        setattr(cfg, k, v)
    cfg.gemm_cfg = -1
    cfg.world_size = 1
    cfg.n_hidden = n_hidden
    return cfg


def _layout(cfg):
    from oac_amd import _lib
    L = _lib.lib()
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) == 0, L.oac_last_error()
    return lay


def _fields(lay):
    return {n: getattr(lay, n) for n, _ in lay._fields_}


def test_abi_version_unchanged():
    from oac_amd import _lib
    assert _lib.lib().oac_abi_version() == 3


@pytest.mark.parametrize("kind,q_out", [(2, 2), (3, 10)])
@pytest.mark.parametrize("dims", [(1, 1, 16), (5, 2, 24), (7, 5, 52)])
@pytest.mark.parametrize("batch", [32, 1100])
def test_depth_1_layout(kind, q_out, dims, batch):
    Do, Da, H = dims
    lay = _layout(_cfg(kind, Do, Da, H, q_out, 1, batch))
    assert lay.pol_fc1_w == -1 and lay.pol_fc1_b == -1
    assert lay.q_fc1_w == -1 and lay.q_fc1_b == -1
    al4 = lambda n: (n + 3) // 4 * 4
    # tensors in order, each 16-byte aligned, nothing between them but padding
    assert (lay.pol_fc0_w, lay.pol_fc0_b) == (0, al4(H * Do))
    assert lay.pol_head_w == lay.pol_fc0_b + al4(H)
    assert lay.pol_head_b == lay.pol_head_w + al4(2 * Da * H)
    assert lay.pol_size == lay.pol_head_b + al4(2 * Da)
    assert (lay.q_fc0_w, lay.q_fc0_b) == (0, al4(H * (Do + Da)))
    assert lay.q_last_w == lay.q_fc0_b + al4(H)
    assert lay.q_last_b == lay.q_last_w + al4(q_out * H)
    assert lay.q_size == lay.q_last_b + al4(q_out)
    for name, v in _fields(lay).items():
        if name.endswith(("_w", "_b", "_size", "_base")) and v >= 0:
            assert v % 4 == 0, (name, v)
    # [policy | target_policy | critic]; one target critic
    assert (lay.tpol_base, lay.q1_base) == (lay.pol_size, 2 * lay.pol_size)
    assert lay.params_total == 2 * lay.pol_size + lay.q_size and lay.targets_total == lay.q_size
    two = _layout(_cfg(kind, Do, Da, H, q_out, 2, batch))
    assert two.pol_size == lay.pol_size + al4(H * H) + al4(H)
    assert two.q_size == lay.q_size + al4(H * H) + al4(H)
    assert lay.workspace_floats > 0


@pytest.mark.parametrize("kind,q_out", [(0, 1), (1, 5), (2, 2), (3, 10), (4, 1)])
def test_n_hidden_0_is_two_layers(kind, q_out):
    a = _fields(_layout(_cfg(kind, 11, 3, 32, q_out, 0)))
    b = _fields(_layout(_cfg(kind, 11, 3, 32, q_out, 2)))
    assert a == b
    assert a["pol_fc1_w"] > 0 and a["q_fc1_w"] > 0


@pytest.mark.parametrize("kind,q_out,name", [(0, 1, b"SAC"), (1, 5, b"PARTICLE"), (4, 1, b"DDPG")])
def test_depth_1_is_rejected_for_the_other_kinds_by_name(kind, q_out, name):
    from oac_amd import _lib
    L = _lib.lib()
    cfg = _cfg(kind, 11, 3, 32, q_out, 1)
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) != 0
    msg = L.oac_last_error()
    assert b"n_hidden" in msg and name in msg and (b"kind %d" % kind) in msg, msg
    assert b"GAUSS" in msg and b"PARTICLE_UB" in msg, msg
    # oac_sac_create validates the same config before it touches a buffer
    bufs = _lib.SacBuffers()
    h = ctypes.c_void_p()
    assert L.oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h)) != 0
    assert name in L.oac_last_error() and not h.value


def test_depth_1_needs_a_hidden_width_of_a_multiple_of_4():
    from oac_amd import _lib
    L = _lib.lib()
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(_cfg(2, 3, 2, 18, 2, 1)), ctypes.byref(lay)) != 0
    msg = L.oac_last_error()
    assert b"multiple of 4" in msg and b"18" in msg, msg
    assert L.oac_sac_query_layout(ctypes.byref(_cfg(2, 3, 2, 18, 2, 2)), ctypes.byref(lay)) == 0


@pytest.mark.parametrize("n_hidden", [-1, 3])
def test_other_depths_are_rejected(n_hidden):
    from oac_amd import _lib
    L = _lib.lib()
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(_cfg(2, 11, 3, 32, 2, n_hidden)),
                                  ctypes.byref(lay)) != 0
    assert b"n_hidden" in L.oac_last_error()
