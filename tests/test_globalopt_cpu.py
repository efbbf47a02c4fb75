"""``global_opt`` off the GPU: the index form of the reference's aliasing
``random.shuffle`` (utils/core.py:74), the CPU restatement of the option
against the reference's own runs (tests/golden/*_go_*.npz), and the C ABI's
config field."""
import ctypes
import random

import numpy as np
import pytest
import torch

import globalopt_lib as gl
import parity
import test_oracle_golden as tog


# ------------------------------------------------------------ the shuffle
@pytest.mark.parametrize("n", [2, 37, 1100])
def test_index_form_of_the_reference_shuffle(n):
    """idx = idx[J] names the rows random.shuffle leaves in a 2-D numpy array
    (it duplicates rows: the swap's right-hand side is two views), over five
    cumulative iterations, and leaves the global random stream where five
    shuffles of an n-row array leave it."""
    from oac_amd.tp_trainer import shuffle_gather_indices
    data = np.random.RandomState(n).randn(n, 3)
    random.seed(1234 + n)
    ref = data.copy()
    want = []
    for _ in range(5):
        random.shuffle(ref)
        want.append(ref.copy())
    state = random.getstate()
    random.seed(1234 + n)
    idx = np.arange(n)
    for k in range(5):
        J = shuffle_gather_indices(n)
        assert J[0] == 0 and np.all(J <= np.arange(n))
        idx = idx[J]
        assert np.array_equal(data[idx], want[k]), k
    assert random.getstate() == state
    if n == 1100:   # the quirk: rows are lost, not permuted
        assert len(np.unique(idx)) < n // 2


def test_index_column_shuffle_equals_data_shuffle():
    """The fixtures' recorded rows: shuffling an index column the reference's
    way gives the rows of shuffling the data."""
    n = 37
    data = np.random.RandomState(0).randn(n, 2)
    random.seed(7)
    ref = data.copy()
    random.shuffle(ref)
    random.shuffle(ref)
    random.seed(7)
    rows = gl.reference_shuffle_indices(n, 2)
    assert np.array_equal(data[rows[1]], ref)


# ------------------------------------------------- restatement vs reference
@pytest.mark.parametrize("name", gl.FIXTURES)
def test_restatement_matches_reference_golden(name):
    """Train steps (policy untouched), every sweep iteration's gradient, loss
    and grad norm, the parameters and the policy optimizer's state after each
    call, under the project's gate with no element excluded."""
    meta, g = parity.load(name)
    assert meta["global_opt"] and meta["n_replay"] == 1100
    for s in range(meta["steps"]):
        assert "Policy Loss" not in [str(k) for k in g[f"s{s}/stat_keys"]]
    assert [int(g[f"c{c}/opt/step"]) for c in range(2)] == [4, 7]
    # the recorded rows are the quirk's: the multiset shrinks with every shuffle
    distinct = [len(np.unique(g[f"c0/i{k}/rows"])) for k in range(4)]
    assert distinct == sorted(distinct, reverse=True) and distinct[0] < 1100
    errs = gl.restatement_errors(meta, g)
    noise = gl.restatement_errors(meta, g, torch.float64)
    assert any(k.startswith("c1/i2/grad/policy/") for k in errs)
    bad = tog.gated(errs, noise)
    print(name, "worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


def test_second_call_restarts_from_init_policy():
    """core.py:68: the policy restarts from init_policy at every call, the
    optimizer's moments and step count carry on."""
    meta, g = parity.load("goac_go_d1")
    rs = gl.Restatement(meta, g=g)
    data = gl.dataset_of(meta)
    rs.sweep(data, [g[f"c0/i{k}/rows"] for k in range(4)])
    assert rs.orc.opt_p.t == 4
    m = {k: v.clone() for k, v in rs.orc.opt_p.m.items()}
    rs.sweep(data, [])
    for k, v in rs.init.items():
        assert torch.equal(rs.orc.P[k], v)
        assert torch.equal(rs.orc.opt_p.m[k], m[k])
    assert rs.orc.opt_p.t == 4


# -------------------------------------------------------------------- ABI
def _cfg(kind, q_out, **kw):
    from oac_amd import _lib
    from oac_amd.trainer import row_layout
    c = _lib.SacConfig()
    c.kind, c.obs_dim, c.act_dim, c.hidden, c.q_out, c.batch = kind, 3, 2, 16, q_out, 8
    c.discount, c.reward_scale, c.tau = 0.99, 1.0, 5e-3
    c.policy_lr = c.qf_lr = 1e-3
    c.beta1, c.beta2, c.adam_eps = 0.9, 0.999, 1e-8
    c.target_update_period, c.world_size, c.gemm_cfg = 1, 1, -1
    for k, v in row_layout(3, 2).items():
        setattr(c, k, v)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _layout(c):
    from oac_amd import _lib
    lay = _lib.SacLayout()
    rc = _lib.lib().oac_sac_query_layout(ctypes.byref(c), ctypes.byref(lay))
    return rc, lay, _lib.lib().oac_last_error().decode()


def test_abi_global_opt_field():
    from oac_amd import _lib
    assert _lib.lib().oac_abi_version() == 3
    assert _lib.SacConfig._fields_[-1][0] == "global_opt" and _lib.SacConfig().global_opt == 0
    names = {_lib.OAC_KIND_SAC: "SAC", _lib.OAC_KIND_PARTICLE: "PARTICLE",
             _lib.OAC_KIND_DDPG: "DDPG"}
    for kind, name in names.items():
        q_out = 4 if kind == _lib.OAC_KIND_PARTICLE else 1
        assert _layout(_cfg(kind, q_out))[0] == 0
        rc, _, err = _layout(_cfg(kind, q_out, global_opt=1))
        assert rc != 0 and "global_opt" in err and name in err, err
    for kind, q_out in ((_lib.OAC_KIND_GAUSS, 2), (_lib.OAC_KIND_PARTICLE_UB, 10)):
        rc, _, err = _layout(_cfg(kind, q_out, global_opt=1, world_size=2))
        assert rc != 0 and "global_opt" in err and "world_size 2" in err, err
        rc, _, err = _layout(_cfg(kind, q_out, global_opt=2))
        assert rc != 0 and "global_opt" in err
        # the parameter layout is the same with and without the field, at both depths
        for depth in (1, 2):
            rc0, lay0, _ = _layout(_cfg(kind, q_out, n_hidden=depth))
            rc1, lay1, _ = _layout(_cfg(kind, q_out, n_hidden=depth, global_opt=1))
            assert rc0 == 0 and rc1 == 0
            for f, _t in _lib.SacLayout._fields_:
                if f != "workspace_floats":   # (the sweep's partials live in the workspace)
                    assert getattr(lay0, f) == getattr(lay1, f), f
            assert lay1.workspace_floats >= lay0.workspace_floats
