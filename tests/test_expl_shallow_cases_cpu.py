"""The input conditions of tests/expl_shallow_cases.py, asserted on the float64
oracle for every case and every row (no GPU; no row is ever dropped), the fp32
oracle's distance from the float64 one (the ref_noise of the GPU gates), and
the host-only side of oac_expl_create_shallow: its dimension refusals, the form
query and the K-head refusal."""
import ctypes

import numpy as np
import pytest

import expl_shallow_cases as ec

# a layer-0 pre-activation this close to 0 (relative to the layer's rms), critics
# this close together, or a gradient this small under the policy's covariance
# would make the ReLU mask / the sign of Q1 - Q2 / the direction of the shift
# depend on fp32 summation order
RELU_MARGIN = 2e-5
GAP = 1e-3
GRAD_NORM = 1e-3

IDS = [c.name for c in ec.ALL_CASES]


def test_case_table_covers_the_issue():
    want = [(1, 1, 8), (1, 1, 16), (5, 2, 24), (23, 6, 252), (300, 18, 256), (513, 4, 64),
            (17, 63, 96), (376, 17, 512)]
    assert ec.DIMS == want and ec.DELTAS == (23.53, 0.5) and ec.BETA_UB == 4.66
    assert ec.PARAM_SEED == 3
    names = set(IDS)
    for delta in ec.DELTAS:
        for Do, Da, H in want:
            c = ec.BY_NAME[f"{Do}x{Da}x{H}-d{delta:g}"]
            assert c.n == 16 and c.seed == Do * 1000 + Da * 10 + H
            assert H % 4 == 0 and H <= 512 and Da <= 63
        for e in ("logstd", "zeroq"):
            assert f"23x6x252-{e}-d{delta:g}" in names
    assert ec.BATCH_CASE.n == 257 and ec.BATCH_NS == (2, 16, 257)


@pytest.mark.parametrize("name", IDS)
def test_input_conditions_hold_for_every_row(name):
    c = ec.BY_NAME[name]
    ref = ec.reference(c)
    for k in ec.OUTPUTS:
        assert ref[k].shape == (c.n, c.Da) and np.isfinite(ref[k]).all(), k
    pre_p, critics = ec.forward64(c)
    worst = np.inf
    for who, pre in (("policy", pre_p), ("critic 1", critics[0][0]), ("critic 2", critics[1][0])):
        rms = np.sqrt(np.mean(pre * pre, axis=1, keepdims=True))
        m = np.abs(pre) / rms
        worst = min(worst, float(m.min()))
        bad = np.nonzero((m < RELU_MARGIN).any(axis=1))[0]
        assert bad.size == 0, (name, who, "rows", bad.tolist())
    q1, q2 = critics[0][1], critics[1][1]
    gap = np.abs(q1 - q2) / np.maximum(np.abs(q1), np.abs(q2))
    assert (gap >= GAP).all(), (name, np.nonzero(gap < GAP)[0].tolist())
    norm = np.sqrt(np.sum(ref["grad"] ** 2 * ref["std"] ** 2, axis=1))
    if c.edge == "zeroq":
        assert not ref["grad"].any() and np.array_equal(ref["mu_E"], ref["mu_T"])
    else:
        assert (norm >= GRAD_NORM).all(), (name, np.nonzero(norm < GRAD_NORM)[0].tolist())
    if c.edge == "logstd":   # both sides of the clamp [-20, 2] are hit
        assert np.allclose(ref["std"][:, 0::2], np.exp(2.0), rtol=1e-12)
        assert np.allclose(ref["std"][:, 1::2], np.exp(-20.0), rtol=1e-12)
    print(f"{name}: relu margin {worst:.2e} twin gap {gap.min():.2e} sqrt(g'Sg) {norm.min():.2e}")


def test_fp32_oracle_distance_is_recorded():
    """ref_noise per case and output (printed: pytest -s): finite everywhere,
    and far below the 1e-5 rule on std (no cancellation there)."""
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


# ------------------------------------------------------------- host-only ABI
def _fake_handle(L, dims, n=1):
    """A handle over host buffers: create stores the pointers and makes no GPU
    call, and the form query reads none of them."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.c_void_p()
    rc = L.lib().oac_expl_create_shallow(n, *dims, p, p, p, p, p, ctypes.c_uint64(1), ctypes.byref(h))
    return rc, h, buf


def test_form_query_reports_the_one_hidden_layer_kernel():
    """*kernel = 2, *group = 1, no write-through form; the observation travels
    in the kernel arguments exactly for the single-observation call with
    obs_dim <= 512."""
    from oac_amd import _lib as L
    for c in ec.CASES:
        for n in (1, c.n):
            rc, h, _buf = _fake_handle(L, (c.Do, c.Da, c.H), n=n)
            assert rc == 0, (c.name, L.lib().oac_last_error())
            try:
                for single_call in (0, 1):
                    v = [ctypes.c_int(-1) for _ in range(4)]
                    L.check(L.lib().oac_expl_launch_form(h, single_call, *[ctypes.byref(x) for x in v]))
                    kernel, group, wt, obs_arg = (x.value for x in v)
                    assert (kernel, group, wt) == (2, 1, 0), (c.name, n, single_call)
                    assert obs_arg == int(single_call == 1 and n == 1 and c.Do <= 512)
                L.check(L.lib().oac_expl_launch_form(h, 0, None, None, None, None))
                assert L.lib().oac_expl_set_ub_index(h, 0) != 0
                msg = L.lib().oac_last_error()
                assert b"oac_expl_set_ub_index" in msg and b"one-hidden-layer" in msg and b"K-head" in msg
                assert L.lib().oac_expl_set_ub_index(h, -1) != 0
            finally:
                assert L.lib().oac_expl_destroy(h) == 0


def test_workspace_size_is_the_batch_handles():
    from oac_amd import _lib as L
    for n, Do, Da, H in ((1, 1, 1, 16), (257, 376, 17, 512)):
        assert L.lib().oac_expl_workspace_floats_batch(n, Do, Da, H) >= n * (Do + Da) + 4 * n * Da + 2


def test_unsupported_dimensions_fail_at_create_by_name():
    """Accepted: hidden % 4 == 0, hidden <= 512, act_dim <= 63, any obs_dim the
    two-layer forms take; anything else is refused at create, by name, before
    any launch."""
    from oac_amd import _lib as L
    for dims, word in (((1, 0, 8), b"act_dim"), ((1, 64, 8), b"act_dim"), ((0, 1, 8), b"obs_dim"),
                       ((1, 1, 0), b"hidden"), ((1, 1, 18), b"hidden"), ((1, 1, 516), b"hidden"),
                       ((1, 1, 2), b"hidden"), ((20000, 2, 64), b"obs_dim")):
        rc, h, _buf = _fake_handle(L, dims)
        msg = L.lib().oac_last_error()
        assert rc != 0 and word in msg and b"one hidden layer" in msg, (dims, msg)
        assert not h.value
    for n in (0, 65537):
        rc, h, _buf = _fake_handle(L, (1, 1, 8), n=n)
        assert rc != 0 and b"n_obs" in L.lib().oac_last_error()
    h = ctypes.c_void_p()
    assert L.lib().oac_expl_create_shallow(1, 1, 1, 8, None, None, None, None, None, ctypes.c_uint64(1),
                                           ctypes.byref(h)) != 0
    assert b"null pointer" in L.lib().oac_last_error()
    for dims in ((1, 1, 4), (1, 1, 512), (1, 63, 8)):   # the limits themselves are taken
        rc, h, _buf = _fake_handle(L, dims)
        assert rc == 0, (dims, L.lib().oac_last_error())
        assert L.lib().oac_expl_destroy(h) == 0
