"""The one-hidden-layer exploration kernel (csrc/expl_shallow.hip) through an
``oac_amd.ShallowSACTrainer`` against the float64 oracle:
tests/expl_shallow_cases.py's table -- the dims from the riverswim recipes to
Humanoid at 512 units, both deltas, the clamp and zero-gradient parameter sets
-- at 1 and 16 observations per call, through both call forms
(oac_expl_action_now and the captured-graph oac_expl_action), a row alone
bitwise the row among N, the form query, the eps-free Philox call, and the
reference's own recordings (tests/golden/oac_expl_d1_*.npz) through
get_optimistic_exploration_action and rollout.

Every output of every row is gated by parity.gate(key, ref_noise) = max(1e-5,
3 * ref_noise), ref_noise the fp32 oracle's distance from the float64 one for
the case (expl_shallow_cases.ref_noise), never a GPU figure."""
import ctypes

import numpy as np
import pytest
import torch

import expl_shallow_cases as ec
import parity
import sac_shallow_lib as ssl
from oracle.philox_oracle import philox_normal

pytestmark = pytest.mark.gpu

_TRAINERS = {}   # params_key -> trainer
_SINGLE = {}     # (case name, row) -> the single-observation call's outputs


def _lib():
    from oac_amd import _lib as L
    return L


def trainer_for(case):
    key = case.params_key
    if key not in _TRAINERS:
        m = dict(obs_dim=case.Do, act_dim=case.Da, hidden=[case.H], discount=0.99, reward_scale=1.0,
                 lr=3e-4, tau=5e-3, auto_alpha=True, log_alpha0=0.0)
        _TRAINERS[key] = ssl.trainer_for(m, params=ec.params_of(key))
    return _TRAINERS[key]


def launch_form(tr, n, single_call):
    L = _lib()
    v = [ctypes.c_int(-1) for _ in range(4)]
    L.check(L.lib().oac_expl_launch_form(tr._expl_handle(n).handle, int(single_call),
                                         *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _kw(case, tr):
    return dict(policy=tr.policy, qfs=tr.qfs,
                hyper_params=dict(beta_UB=ec.BETA_UB, delta=case.delta, share_layers=False))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run(case, tr, obs, eps):
    """One call on obs [n, Do] (n = 1: the single-observation entry point):
    action, mu_E, std from oac_expl_action_now (return_info=True); all four
    outputs from oac_expl_action on the same handle (the captured-graph form:
    its staging still holds the call's observations, its eps slot the call's
    eps), whose action / mu_E / std must be bitwise the first call's."""
    from oac_amd import get_optimistic_exploration_action, get_optimistic_exploration_actions
    L = _lib()
    n, Da = obs.shape[0], case.Da
    kw = _kw(case, tr)
    if n == 1:
        a, info = get_optimistic_exploration_action(obs[0], eps=eps[0], return_info=True, **kw)
        out = dict(action=a[None, :], mu_E=info["mu_E"][None, :], std=info["std"][None, :])
    else:
        A, info = get_optimistic_exploration_actions(obs, eps=eps, return_info=True, **kw)
        out = dict(action=A, mu_E=info["mu_E"], std=info["std"])
    e = tr._expl_handle(n)
    s = torch.cuda.current_stream(tr.device)
    g = torch.full((4, n, Da), float("nan"), dtype=torch.float32, device=tr.device)
    L.check(L.lib().oac_expl_action(e.handle, L.ptr(e.eps), float(ec.BETA_UB), float(case.delta),
                                    L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(g[3]),
                                    L.stream_ptr(s)))
    s.synchronize()
    g = g.cpu().numpy()
    for i, k in enumerate(("action", "mu_E", "std")):
        assert out[k].dtype == np.float32 and out[k].shape == (n, Da)
        assert _bits_equal(g[i], out[k]), (case.name, n, k, "oac_expl_action != oac_expl_action_now")
        assert _bits_equal(e.out_np[i], out[k]), (case.name, n, k, "the graph's pinned download")
    out["grad"] = g[3]
    return out


def compare(case, got, rows, what):
    """Every output of every row of ``got`` (rows: their indices in the case's
    draw) against the float64 oracle; prints the worst figures, then asserts."""
    ref, noise = ec.reference(case), ec.ref_noise(case)
    bad, worst = [], {}
    for k in ec.OUTPUTS:
        gate = parity.gate(k, noise[k])
        assert np.isfinite(got[k]).all(), (case.name, what, k)
        for j, r in enumerate(rows):
            if k == "grad" and case.edge == "zeroq":
                # the reference is exactly 0: absolute, against the scale of dQ/da
                err = float(np.abs(got[k][j]).max()) / ec.w0_action_rms(case)
                lim = 1e-6
            else:
                err, lim = parity.rel_err(got[k][j], ref[k][r]), gate
            if err >= worst.get(k, (-1.0,))[0]:
                worst[k] = (err, r)
            if not err <= lim:
                bad.append((k, r, err, lim))
    print(f"  {case.name} {what}: " + " ".join(
        f"{k} {worst[k][0]:.2e}@{worst[k][1]} (ref_noise {noise[k]:.1e})" for k in ec.OUTPUTS))
    assert not bad, (case.name, what, sorted(bad, key=lambda b: -b[2] / b[3])[:8])


def single_rows(case, tr, rows):
    obs, eps = ec.inputs(case)
    for r in rows:
        if (case.name, r) not in _SINGLE:
            _SINGLE[(case.name, r)] = run(case, tr, obs[r:r + 1], eps[r:r + 1])
    return {k: np.concatenate([_SINGLE[(case.name, r)][k] for r in rows]) for k in ec.OUTPUTS}


@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_case_matches_float64_oracle_at_1_and_16_rows(name):
    """n = 16 in one call and each of its rows as a single call, each through
    both call forms: every output of every row within parity.gate of the
    float64 oracle, and the batched row bitwise the single call (host rows and
    the completion word against the observation argument and tagged granules).
    (17, 63, 96): a trainer with act_dim > 32 is built for exploration alone."""
    case = ec.BY_NAME[name]
    tr = trainer_for(case)
    obs, eps = ec.inputs(case)
    rows = list(range(case.n))
    for n in (1, case.n):
        for sc in (1, 0):
            k, g, wt, oa = launch_form(tr, n, sc)
            assert (k, g, wt) == (2, 1, 0), (name, n, sc)
            assert oa == int(sc == 1 and n == 1 and case.Do <= 512)
    batch = run(case, tr, obs, eps)
    single = single_rows(case, tr, rows)
    compare(case, batch, rows, f"n={case.n}")
    compare(case, single, rows, "n=1")
    for k in ec.OUTPUTS:
        for r in rows:
            assert _bits_equal(batch[k][r], single[k][r]), (name, k, "row", r, batch[k][r], single[k][r])
    if case.edge == "zeroq":
        assert not batch["grad"].any() and not single["grad"].any()


@pytest.mark.parametrize("n", ec.BATCH_NS)
def test_a_row_alone_is_bitwise_the_row_among_n(n):
    """The first n rows of the 257-row draw in one call (257 workgroups in one
    launch): every row against float64, rows {0, 1, n // 2, n - 1} bitwise the
    single call."""
    case = ec.BATCH_CASE
    tr = trainer_for(case)
    obs, eps = ec.inputs(case)
    got = run(case, tr, obs[:n], eps[:n])
    compare(case, got, list(range(n)), f"n={n}")
    rows = sorted({0, 1, n // 2, n - 1})
    single = single_rows(case, tr, rows)
    for k in ec.OUTPUTS:
        for j, r in enumerate(rows):
            assert _bits_equal(got[k][r], single[k][j]), (n, k, "row", r)


@pytest.mark.parametrize("name", ["1x1x16-d23.53", "513x4x64-d0.5"])
def test_eps_free_call_draws_philox_noise(name):
    """eps = NULL: the single call (tagged form at (1, 1, 16), host row at
    (513, 4, 64)) advances step_state[2] by one, equals the N = 1 batched
    Philox call at the same counter, and is the call fed the oracle's float32
    Philox draws -- philox_normal(seed + 1, counter, 3, j), the two-layer
    handle's contract (mu_E and std bitwise, the action within std * 4 |d eps|
    + 2^-21, as tests/test_gpu_expl_shapes.py)."""
    from oac_amd import get_optimistic_exploration_action, get_optimistic_exploration_actions
    case = ec.BY_NAME[name]
    tr = trainer_for(case)
    obs, _ = ec.inputs(case)
    kw = _kw(case, tr)
    assert launch_form(tr, 1, 1)[3] == int(case.Do <= 512)
    tr.step_state[2] = 7
    a1, info = get_optimistic_exploration_action(obs[0], **kw)
    assert info == {} and a1.shape == (case.Da,) and a1.dtype == np.float32
    assert int(tr.step_state[2].item()) == 8
    out = tr._expl_handle(1).out_np.copy()
    a2, _ = get_optimistic_exploration_action(obs[0], **kw)
    assert int(tr.step_state[2].item()) == 9
    assert np.isfinite(a1).all() and not np.array_equal(a1, a2)
    tr.step_state[2] = 7
    A, _ = get_optimistic_exploration_actions(obs[:1], **kw)
    assert _bits_equal(A[0], a1) and int(tr.step_state[2].item()) == 8
    # rows of a batched call take elements r * Da + j of the call's one counter
    tr.step_state[2] = 7
    A3, _ = get_optimistic_exploration_actions(obs[:3], **kw)
    assert _bits_equal(A3[0], a1) and int(tr.step_state[2].item()) == 8
    idx = np.arange(case.Da)
    e32 = philox_normal(tr.seed + 1, 7, 3, idx, np.float32)
    d_eps = np.abs(e32.astype(np.float64) - philox_normal(tr.seed + 1, 7, 3, idx, np.float64)).max()
    fed, finfo = get_optimistic_exploration_action(obs[0], eps=e32, return_info=True, **kw)
    assert _bits_equal(finfo["mu_E"], out[1, 0]) and _bits_equal(finfo["std"], out[2, 0])
    allow = finfo["std"].astype(np.float64) * (4 * d_eps) + 2.0 ** -21
    d = np.abs(a1.astype(np.float64) - fed.astype(np.float64))
    print(f"  max |a_free - a_fed| {d.max():.3e}, {float((d / allow).max()):.3f} of the allowance")
    assert (d <= allow).all()


@pytest.mark.parametrize("name", ssl.EXPL_FIXTURES)
def test_exploration_matches_reference_golden(name):
    """The reference's own recordings through get_optimistic_exploration_action
    (single calls) and get_optimistic_exploration_actions (all 16 at once,
    bitwise the single calls)."""
    from oac_amd import get_optimistic_exploration_action, get_optimistic_exploration_actions
    meta, g = parity.load(name)
    m = dict(obs_dim=meta["obs_dim"], act_dim=meta["act_dim"], hidden=meta["hidden"], discount=0.99,
             reward_scale=1.0, lr=3e-4, tau=5e-3, auto_alpha=True, log_alpha0=0.0, seed=meta["seed"],
             pi_init_w=meta["pi_init_w"], q_init_w=meta["q_init_w"])
    tr = ssl.trainer_for(m)
    hp = dict(beta_UB=meta["beta_UB"], delta=meta["delta"], share_layers=False)
    A, infos = get_optimistic_exploration_actions(g["obs"], policy=tr.policy, qfs=tr.qfs,
                                                  hyper_params=hp, eps=g["eps"], return_info=True)
    for i in range(meta["n_obs"]):
        a, info = get_optimistic_exploration_action(g["obs"][i], policy=tr.policy, qfs=tr.qfs,
                                                    hyper_params=hp, eps=g["eps"][i], return_info=True)
        assert a.dtype == np.float32 and a.shape == (meta["act_dim"],)
        assert parity.rel_err(info["std"], g["std"][i]) <= parity.TOL
        assert parity.rel_err(info["mu_E"], g["mu_E"][i]) <= parity.TOL
        assert parity.rel_err(a, g["action"][i]) <= parity.TOL
        assert _bits_equal(A[i], a) and _bits_equal(infos["mu_E"][i], info["mu_E"])


class _FixtureEnv:
    """Starts at a recorded observation; the next ones depend on the actions."""

    def __init__(self, o0, length):
        self.o0, self.length = np.asarray(o0, np.float64), length

    def reset(self):
        self.t, self.o = 0, self.o0.copy()
        return self.o.copy()

    def step(self, a):
        self.t += 1
        a = np.asarray(a, np.float64)
        self.o = np.tanh(self.o + np.resize(a, self.o.shape) * 0.5)
        return self.o.copy(), float(a.sum()), self.t >= self.length, {"t": self.t}


@pytest.mark.parametrize("name", ssl.EXPL_FIXTURES)
def test_rollout_through_a_shallow_trainer_matches_the_fixture(name):
    """vec_rollout with a ShallowSACTrainer's policy and critics: the first
    step from the fixture's 16 observations with the fixture's noise gives the
    reference's recorded actions; and with fixed noise every environment's
    path is bitwise the single-environment loop of path_collector.rollout
    (one get_optimistic_exploration_action call per step)."""
    from oac_amd import get_optimistic_exploration_action, vec_rollout
    from test_rollout import _same, walk
    meta, g = parity.load(name)
    m = dict(obs_dim=meta["obs_dim"], act_dim=meta["act_dim"], hidden=meta["hidden"], discount=0.99,
             reward_scale=1.0, lr=3e-4, tau=5e-3, auto_alpha=True, log_alpha0=0.0, seed=meta["seed"],
             pi_init_w=meta["pi_init_w"], q_init_w=meta["q_init_w"])
    tr = ssl.trainer_for(m)
    hp = dict(beta_UB=meta["beta_UB"], delta=meta["delta"], share_layers=False)
    n, Da = meta["n_obs"], meta["act_dim"]
    paths = vec_rollout([_FixtureEnv(g["obs"][i], 1) for i in range(n)], tr.policy, max_path_length=1,
                        optimistic_exploration=True,
                        optimistic_exploration_kwargs=dict(policy=tr.policy, qfs=tr.qfs, hyper_params=hp,
                                                           eps=g["eps"]))
    for i in range(n):
        assert paths[i]["actions"].shape == (1, Da)
        np.testing.assert_array_equal(paths[i]["observations"][0], g["obs"][i])
        assert parity.rel_err(paths[i]["actions"][0], g["action"][i]) <= parity.TOL
    kw = dict(policy=tr.policy, qfs=tr.qfs, hyper_params=hp, eps=np.full(Da, 0.25, np.float32))
    lengths = [3, 7, 7, 20]
    paths = vec_rollout([_FixtureEnv(g["obs"][s], L) for s, L in enumerate(lengths)], tr.policy,
                        max_path_length=16, optimistic_exploration=True,
                        optimistic_exploration_kwargs=kw)
    for s, L in enumerate(lengths):
        ref = walk(_FixtureEnv(g["obs"][s], L),
                   lambda o: get_optimistic_exploration_action(o, **kw)[0], 16)
        _same(paths[s], ref)
