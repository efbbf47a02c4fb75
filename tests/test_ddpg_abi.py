"""CPU checks of the C-ABI boundary for OAC_KIND_DDPG: the arena layout facts
(host-side layout logic, no GPU compute)."""
import ctypes

import pytest


def _cfg(Do, Da, H, q_out=1, batch=256):
    from oac_amd import _lib, row_layout
    cfg = _lib.SacConfig()
    cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = (
        _lib.OAC_KIND_DDPG, Do, Da, H, q_out, batch)
    for k, v in row_layout(Do, Da).items():
        setattr(cfg, k, v)
    cfg.gemm_cfg = -1
    cfg.world_size = 1
    return cfg


@pytest.mark.parametrize("dims", [(376, 17, 256), (11, 3, 16)])
def test_ddpg_layout(dims):
    """params / grads / m / v = [policy | critic], targets = [target critic]:
    one critic, no second critic, no target_policy block."""
    from oac_amd import _lib
    assert _lib.OAC_KIND_DDPG == 4
    Do, Da, H = dims
    L = _lib.lib()
    assert L.oac_abi_version() == 3
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(_cfg(Do, Da, H)), ctypes.byref(lay)) == 0, \
        L.oac_last_error()
    assert lay.n_critics == 1
    assert lay.q2_base < 0
    assert lay.tpol_base == -1
    assert lay.q1_base == lay.pol_size
    assert lay.params_total == lay.pol_size + lay.q_size
    assert lay.targets_total == lay.q_size
    n_pol = H * Do + H + H * H + H + 2 * (Da * H + Da)
    n_q = H * (Do + Da) + H + H * H + H + H + 1
    assert lay.pol_size >= n_pol and lay.pol_size - n_pol < 4 * 6
    assert lay.q_size >= n_q and lay.q_size - n_q < 4 * 6
    assert lay.q_last_b - lay.q_last_w >= H        # q_out == 1: one last-layer row
    assert lay.workspace_floats > 0
    # the SAC layout of the same dims has the second critic the DDPG one lacks
    sac = _cfg(Do, Da, H)
    sac.kind = _lib.OAC_KIND_SAC
    lay2 = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(sac), ctypes.byref(lay2)) == 0
    assert lay2.params_total == lay.params_total + lay.q_size
    for B in (256, 1024):   # both kernel sets lay a workspace out
        lay3 = _lib.SacLayout()
        assert L.oac_sac_query_layout(ctypes.byref(_cfg(Do, Da, H, batch=B)), ctypes.byref(lay3)) == 0
        assert lay3.workspace_floats > 0


@pytest.mark.parametrize("q_out", [0, 2, 5])
def test_ddpg_bad_q_out_is_rejected_with_a_message(q_out):
    from oac_amd import _lib
    L = _lib.lib()
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(_cfg(11, 3, 16, q_out=q_out)), ctypes.byref(lay)) != 0
    msg = L.oac_last_error()
    assert b"q_out" in msg and b"DDPG" in msg, msg


def test_kind_7_stays_rejected():
    from oac_amd import _lib
    L = _lib.lib()
    cfg = _cfg(11, 3, 16)
    cfg.kind = 7
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) != 0
    assert b"kind" in L.oac_last_error()


def test_ddpg_is_single_process():
    from oac_amd import _lib
    L = _lib.lib()
    cfg = _cfg(11, 3, 16)
    cfg.world_size = 2
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) != 0
    assert b"DDPG" in L.oac_last_error()
