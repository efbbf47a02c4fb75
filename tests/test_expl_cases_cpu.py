"""The input conditions of tests/expl_cases.py, asserted on the float64
oracle for every case and every row (no GPU): where one fails, the case's
seed changes (expl_cases.SEED_OVERRIDES) -- no row is ever dropped.  The fp32
oracle's distance from the float64 one (the ref_noise of the GPU gates) is
recorded here per case and output."""
import numpy as np
import pytest

import expl_cases as ec

# relative margins (the issue's): a pre-activation this close to 0, critics
# this close together or sorted heads this close to a neighbour would make the
# gradient's ReLU mask / sign / selected head depend on fp32 summation order
RELU_MARGIN = 5e-6
GAP = 1e-4

IDS = [c.name for c in ec.ALL_CASES]


def test_case_table_covers_the_issue():
    assert len(ec.TWIN_DIMS) == 13 and len(ec.HEAD_DIMS) == 4
    names = set(IDS)
    for delta in ec.DELTAS:
        for Do, Da, H in ec.TWIN_DIMS:
            assert f"{Do}x{Da}x{H}-d{delta:g}" in names
        for Do, Da, H, K in ec.HEAD_DIMS:
            di = ec.delta_index(K)
            assert di is not None and 0 <= di <= K - 1
            for b in ("mean", "ub0", f"ub{K - 1}", f"ub{di}"):
                assert f"{Do}x{Da}x{H}x{K}-{b}-d{delta:g}" in names
        for e in ("23x6x250-logstd", "23x6x250-zeroq", "13x6x80x16-mean-logstd"):
            assert f"{e}-d{delta:g}" in names
    assert [c.n for c in ec.SWEEP_CASES] == [257] * 3 and max(ec.SWEEP_NS) == 257
    for c in ec.CASES:
        assert c.n == 16


@pytest.mark.parametrize("name", IDS)
def test_input_conditions_hold_for_every_row(name):
    c = ec.BY_NAME[name]
    ref = ec.reference(c)
    for k in ec.OUTPUTS:
        assert ref[k].shape == (c.n, c.Da) and np.isfinite(ref[k]).all(), k
    worst_relu = np.inf
    for i, (pre0, pre1, q) in enumerate(ec.critic_forward64(c)):
        for layer, pre in enumerate((pre0, pre1)):
            rms = np.sqrt(np.mean(pre * pre, axis=1, keepdims=True))
            m = np.abs(pre) / rms
            worst_relu = min(worst_relu, float(m.min()))
            bad = np.nonzero((m < RELU_MARGIN).any(axis=1))[0]
            assert bad.size == 0, (name, "critic", i, "layer", layer, "rows", bad.tolist())
    cf = ec.critic_forward64(c)
    if c.twin:
        q1, q2 = cf[0][2][:, 0], cf[1][2][:, 0]
        gap = np.abs(q1 - q2) / (np.abs(q1) + np.abs(q2))
        assert (gap >= GAP).all(), (name, np.nonzero(gap < GAP)[0].tolist())
        print(f"{name}: relu margin {worst_relu:.2e} twin gap {gap.min():.2e}")
    elif c.ub is not None:
        s = np.sort(cf[0][2], axis=1)
        sel = s[:, c.ub]
        worst = np.inf
        for nb in (c.ub - 1, c.ub + 1):
            if 0 <= nb < c.K:
                gap = np.abs(sel - s[:, nb]) / (np.abs(sel) + np.abs(s[:, nb]))
                assert (gap >= GAP).all(), (name, nb, np.nonzero(gap < GAP)[0].tolist())
                worst = min(worst, float(gap.min()))
        print(f"{name}: relu margin {worst_relu:.2e} sorted-head gap {worst:.2e}")
    if c.delta == 0.5:
        med = float(np.median(np.abs(ref["action"])))
        assert med < 0.9, (name, med)
    if c.edge == "zeroq":
        assert not ref["grad"].any() and np.array_equal(ref["mu_E"], ref["mu_T"])
    if c.edge == "logstd":   # both sides of the clamp [-20, 2] are hit
        assert np.allclose(ref["std"][:, 0::2], np.exp(2.0), rtol=1e-12)
        if c.Da > 1:
            assert np.allclose(ref["std"][:, 1::2], np.exp(-20.0), rtol=1e-12)


def test_fp32_oracle_distance_is_recorded():
    """ref_noise per case and output (printed: pytest -s); over the whole table
    it stays far below the 1e-5 rule on std (no cancellation there), and is
    finite everywhere."""
    worst = {k: (0.0, None) for k in ec.OUTPUTS}
    for c in ec.ALL_CASES:
        nz = ec.ref_noise(c)
        print(f"ref_noise {c.name}: " + " ".join(f"{k}={nz[k]:.2e}" for k in ec.OUTPUTS))
        for k in ec.OUTPUTS:
            assert np.isfinite(nz[k]) and nz[k] >= 0.0
            if nz[k] > worst[k][0]:
                worst[k] = (float(nz[k]), c.name)
    print("worst ref_noise:", worst)
    assert worst["std"][0] < 1e-5


def _fake_handle(L, dims, K=None, n=1):
    """A handle over host buffers: create stores the pointers and makes no GPU
    call, and the form query reads none of them."""
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.c_void_p()
    if K is None:
        rc = L.lib().oac_expl_create_batch(n, *dims, p, p, p, p, p, ctypes.c_uint64(1),
                                           ctypes.byref(h))
    else:
        rc = L.lib().oac_expl_create_shared(n, *dims, K, p, p, p, p, ctypes.c_uint64(1),
                                            ctypes.byref(h))
    return rc, h, buf


def test_form_query_picks_the_kernel_the_table_expects():
    """oac_expl_launch_form needs no device work: the kernel it reports is the
    one the case table expects on any device -- a budget constant that moves a
    shape to the other kernel fails here.  Without a device it answers one
    workgroup per observation, dynamic LDS, never the observation argument."""
    import ctypes
    import torch
    from oac_amd import _lib as L
    no_device = not torch.cuda.is_available()
    for c in ec.CASES:
        for n in (1, c.n):
            rc, h, _buf = _fake_handle(L, (c.Do, c.Da, c.H), c.K, n=n)
            assert rc == 0, (c.name, L.lib().oac_last_error())
            try:
                for single_call in (0, 1):
                    v = [ctypes.c_int(-1) for _ in range(4)]
                    L.check(L.lib().oac_expl_launch_form(h, single_call,
                                                         *[ctypes.byref(x) for x in v]))
                    kernel, group, wt, obs_arg = (x.value for x in v)
                    assert kernel == int(c.split_kernel), (c.name, n, single_call)
                    assert 1 <= group <= 32 and wt in (0, 1) and obs_arg in (0, 1)
                    assert not wt or group > 1
                    assert not obs_arg or (wt and single_call and n == 1 and c.Do <= 512)
                    if no_device:
                        assert (group, wt, obs_arg) == (1, 0, 0), (c.name, n, single_call)
                L.check(L.lib().oac_expl_launch_form(h, 0, None, None, None, None))
            finally:
                assert L.lib().oac_expl_destroy(h) == 0
    assert L.lib().oac_expl_launch_form(None, 0, None, None, None, None) != 0


def test_unsupported_dimensions_fail_at_create_by_name():
    """A dimension no kernel form takes is refused by oac_expl_create*, with a
    message, before any launch."""
    from oac_amd import _lib as L
    for dims, word in (((1, 0, 8), b"act_dim"), ((1, 64, 8), b"act_dim"), ((0, 1, 8), b"obs_dim"),
                       ((1, 1, 0), b"hidden"), ((8, 2, 2048), b"LDS")):
        rc, h, _buf = _fake_handle(L, dims)
        assert rc != 0 and word in L.lib().oac_last_error(), (dims, L.lib().oac_last_error())
    for K in (1, 17):
        rc, h, _buf = _fake_handle(L, (1, 1, 8), K)
        assert rc != 0 and b"K" in L.lib().oac_last_error()
    rc, h, _buf = _fake_handle(L, (1, 1, 8), n=0)
    assert rc != 0 and b"n_obs" in L.lib().oac_last_error()


def test_gradient_step_refuses_act_dim_past_32_by_name():
    """The parameter layout (and with it the exploration handle) takes act_dim
    up to 63; the gradient step's row kernels give one half-wave lane per
    action dim, so a step plan for more than 32 is refused at create, by name
    (host-only: refused before any buffer is read)."""
    import ctypes
    from oac_amd import _lib as L
    from oac_amd import row_layout
    for Da, ok in ((32, True), (33, False), (63, False)):
        cfg = L.SacConfig()
        cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = 0, 17, Da, 96, 1, 8
        for k, v in row_layout(17, Da).items():
            setattr(cfg, k, v)
        cfg.gemm_cfg, cfg.world_size = -1, 1
        lay = L.SacLayout()
        assert L.lib().oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) == 0
        h = ctypes.c_void_p()
        bufs = L.SacBuffers()
        rc = L.lib().oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h))
        if ok:
            assert rc == 0 and L.lib().oac_sac_destroy(h) == 0
        else:
            assert rc != 0 and b"gradient step takes act_dim <= 32" in L.lib().oac_last_error()
    cfg.act_dim = 64
    assert L.lib().oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) != 0
    assert b"bad dims" in L.lib().oac_last_error()
