"""The exploration kernels (csrc/expl_split.hip) at their shape edges against
the float64 oracle: tests/expl_cases.py's table -- dims at each budget and
remainder, twin critics through the split kernel, K heads with every bound,
both deltas, the clamp and zero-gradient parameter sets -- at 1 and 16
observations per call, a sweep over the observations per launch (group sizes
that do not divide the 32 parts, one workgroup per observation, a second
launch), grad from oac_expl_action, row-of-a-batch == single call bitwise, and
an assertion that all six built forms were run (oac_expl_launch_form).

Every output of every row is gated by parity.gate(key, ref_noise) =
max(1e-5, 3 * ref_noise), ref_noise the fp32 oracle's distance from the
float64 one for the case (expl_cases.ref_noise), never a GPU figure."""
import ctypes

import numpy as np
import pytest
import torch

import expl_cases as ec
import parity
from gpu_helpers import Space, producers, sac_trainer_for
from oracle.philox_oracle import philox_normal

pytestmark = pytest.mark.gpu

FORM_NAMES = {(0, 1, 0): "twin write-through", (0, 0, 0): "twin dynamic-LDS",
              (0, 1, 1): "twin write-through + observation argument",
              (1, 1, 0): "split write-through", (1, 0, 0): "split dynamic-LDS",
              (1, 1, 1): "split write-through + observation argument"}
_FORMS = {}      # (kernel, write_through, obs_in_args) -> first case that ran it
_TRAINERS = {}   # expl_cases params_key -> trainer
_SINGLE = {}     # (case name, row) -> the single-observation call's outputs
_WORST = {}      # output -> (largest error / gate, error, ref_noise, case, row)


def _lib():
    from oac_amd import _lib as L
    return L


def trainer_for(case):
    key = case.params_key
    if key in _TRAINERS:
        return _TRAINERS[key]
    params = ec.params_of(key)
    if case.twin:
        m = dict(obs_dim=case.Do, act_dim=case.Da, hidden=[case.H, case.H], discount=0.99,
                 reward_scale=1.0, lr=3e-4, tau=5e-3, auto_alpha=True, log_alpha0=0.0)
        tr = sac_trainer_for(m, params=params)
    else:
        from oac_amd import ParticleTrainerOAC
        pp, qp = producers(params, q_keys=("qf1", "qf2", "target_qf1", "target_qf2", "qf1",
                                           "target_qf1"))
        tr = ParticleTrainerOAC(pp, qp, n_estimators=case.K, action_space=Space(case.Da),
                                deterministic=False, q_min=0.0, q_max=50.0, share_layers=True,
                                delta=ec.UB_TRAINER_DELTA)
        assert tr.delta_index == ec.delta_index(case.K)
    _TRAINERS[key] = tr
    return tr


def launch_form(tr, n, single_call, who):
    """(kernel, group, write_through, obs_in_args) of the handle's first launch."""
    L = _lib()
    v = [ctypes.c_int(-1) for _ in range(4)]
    L.check(L.lib().oac_expl_launch_form(tr._expl_handle(n).handle, int(single_call),
                                         *[ctypes.byref(x) for x in v]))
    k, g, wt, oa = (x.value for x in v)
    assert k in (0, 1) and 1 <= g <= 32 and wt in (0, 1) and oa in (0, 1)
    _FORMS.setdefault((k, wt, oa), who)
    return k, g, wt, oa


def _form_str(f):
    return f"{FORM_NAMES[(f[0], f[2], f[3])]} G={f[1]}"


def _call_kw(case, tr):
    kw = dict(policy=tr.policy, qfs=tr.qfs,
              hyper_params=dict(beta_UB=ec.BETA_UB, delta=case.delta, share_layers=not case.twin))
    if not case.twin and case.ub is not None:   # --trainer_UB: the head sorted at delta_index
        tr.delta_index = case.ub
        kw["trainer"] = tr
    return kw


def run(case, tr, obs, eps):
    """One call on obs [n, Do] (n = 1: the single-observation entry point):
    action, mu_E, std from return_info=True; grad from oac_expl_action on the
    same handle (the captured-graph path: its staging still holds the call's
    observations, its eps slot the call's eps), whose action / mu_E / std must
    be bitwise the first call's.  {output: float32 [n, Da]}."""
    from oac_amd import get_optimistic_exploration_action, get_optimistic_exploration_actions
    L = _lib()
    n, Da = obs.shape[0], case.Da
    kw = _call_kw(case, tr)
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
    out["grad"] = g[3]
    return out


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


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
            if err / lim > _WORST.get(k, (-1.0,))[0]:
                _WORST[k] = (err / lim, err, noise[k], case.name + " " + what, r)
            if not err <= lim:
                bad.append((k, r, err, lim))
    print(f"  {case.name} {what}: " + " ".join(
        f"{k} {worst[k][0]:.2e}@{worst[k][1]} (ref_noise {noise[k]:.1e})" for k in ec.OUTPUTS))
    assert not bad, (case.name, what, sorted(bad, key=lambda b: -b[2] / b[3])[:8])


def single_rows(case, tr, rows):
    """The single-observation call's outputs on the given rows of the case's
    draw (each computed once)."""
    obs, eps = ec.inputs(case)
    for r in rows:
        if (case.name, r) not in _SINGLE:
            _SINGLE[(case.name, r)] = run(case, tr, obs[r:r + 1], eps[r:r + 1])
    return {k: np.concatenate([_SINGLE[(case.name, r)][k] for r in rows]) for k in ec.OUTPUTS}


@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_case_matches_float64_oracle_at_1_and_16_rows(name):
    """n = 16 in one call and each of its rows as a single call: every output
    of every row within parity.gate of the float64 oracle, and the batched
    row bitwise the single call (another form: 16 against 32 workgroups per
    observation, host rows against the observation argument).

    (29, 33, 64) and (17, 63, 96): a trainer with act_dim > 32 is built for
    exploration alone (its gradient step is refused by name at plan creation).

    Zero-gradient set (critic last_fc.weight = 0): grad is compared
    absolutely, |grad| <= 1e-6 * rms(W0 action columns); measured on MI355X:
    exactly 0 in every row (the seeds multiply zeros), mu_E bitwise mu_T."""
    case = ec.BY_NAME[name]
    tr = trainer_for(case)
    obs, eps = ec.inputs(case)
    rows = list(range(case.n))
    forms = [launch_form(tr, n, sc, name) for n in (1, case.n) for sc in (1, 0)]
    print(f"\n{name}: n=1 now: {_form_str(forms[0])}; n=1 graph: {_form_str(forms[1])}; "
          f"n={case.n} now: {_form_str(forms[2])}; graph: {_form_str(forms[3])}")
    assert [f[0] for f in forms] == [int(case.split_kernel)] * 4, (name, forms)
    batch = run(case, tr, obs, eps)
    single = single_rows(case, tr, rows)
    compare(case, batch, rows, f"n={case.n}")
    compare(case, single, rows, "n=1")
    for k in ec.OUTPUTS:
        for r in rows:
            assert _bits_equal(batch[k][r], single[k][r]), (name, k, "row", r, batch[k][r],
                                                             single[k][r])
    if case.edge == "zeroq":
        assert not batch["grad"].any() and not single["grad"].any()


SWEEP = [(c.name, n) for c in ec.SWEEP_CASES for n in ec.SWEEP_NS] + \
        [(ec.WIDE_CASE.name, n) for n in ec.WIDE_NS]


@pytest.mark.parametrize("name,n", SWEEP)
def test_group_size_sweep(name, n):
    """The first n rows of the shape's 257-row draw in one call: every row
    against float64, rows {0, 1, n // 2, n - 1} bitwise the single call.  On
    256 CUs the groups are 32 / 28 / 21 / 6 / 3 / 2 / 1 / 1 workgroups (the
    form query's figure is printed, not assumed); 129 rows run the
    dynamic-LDS forms, 257 a second launch of one row.  The wide case (H =
    640, twin critics in the split kernel) is where a workgroup owning two
    column parts holds more dh1 columns than 2H / G + 32."""
    case = ec.BY_NAME[name]
    tr = trainer_for(case)
    obs, eps = ec.inputs(case)
    f = launch_form(tr, n, 1, f"{name} n={n}")
    launch_form(tr, n, 0, f"{name} n={n}")
    print(f"\n{name} n={n}: {_form_str(f)}")
    got = run(case, tr, obs[:n], eps[:n])
    compare(case, got, list(range(n)), f"n={n}")
    rows = sorted({0, 1, n // 2, n - 1})
    launch_form(tr, 1, 1, f"{name} n=1")
    launch_form(tr, 1, 0, f"{name} n=1")
    single = single_rows(case, tr, rows)
    for k in ec.OUTPUTS:
        for j, r in enumerate(rows):
            assert _bits_equal(got[k][r], single[k][j]), (name, n, k, "row", r)


@pytest.mark.parametrize("name,obs_arg", [("513x4x64-d0.5", 0), ("300x19x256-d0.5", 1)])
def test_single_call_philox_path_split_kernel(name, obs_arg):
    """The eps-free single call with twin critics in the split kernel: at
    (513, 4, 64) through the host row (no observation argument, no tags), at
    (300, 19, 256) through the tagged form.  It advances step_state[2] by one,
    equals the N = 1 batched Philox call at the same counter, and is the call
    fed the oracle's float32 Philox draws (mu_E and std bitwise, the action
    within std * 4 |d eps| + 2^-21: tanh is 1-Lipschitz, two float32 ulps for
    the roundings of eps * std + mu_E and tanhf, as tests/test_gpu_noise.py)."""
    from oac_amd import get_optimistic_exploration_action, get_optimistic_exploration_actions
    case = ec.BY_NAME[name]
    tr = trainer_for(case)
    obs, _ = ec.inputs(case)
    kw = _call_kw(case, tr)
    f = launch_form(tr, 1, 1, name + " philox")
    print(f"\n{name} eps-free single call: {_form_str(f)}")
    assert (f[0], f[3]) == (1, obs_arg)
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
    assert _bits_equal(A[0], a1)
    assert int(tr.step_state[2].item()) == 8
    idx = np.arange(case.Da)
    e32 = philox_normal(tr.seed + 1, 7, 3, idx, np.float32)
    d_eps = np.abs(e32.astype(np.float64) - philox_normal(tr.seed + 1, 7, 3, idx, np.float64)).max()
    fed, finfo = get_optimistic_exploration_action(obs[0], eps=e32, return_info=True, **kw)
    assert _bits_equal(finfo["mu_E"], out[1, 0]) and _bits_equal(finfo["std"], out[2, 0])
    allow = finfo["std"].astype(np.float64) * (4 * d_eps) + 2.0 ** -21
    d = np.abs(a1.astype(np.float64) - fed.astype(np.float64))
    print(f"  max |a_free - a_fed| {d.max():.3e}, {float((d / allow).max()):.3f} of the allowance")
    assert (d <= allow).all()
    ref = ec.reference(case)
    assert parity.rel_err(finfo["mu_E"], ref["mu_E"][0]) <= parity.gate("mu_E", ec.ref_noise(case)["mu_E"])


def test_zz_every_built_form_was_run():
    """(Last in the module.)  The form query over everything above: all six
    built forms -- each kernel with write-through hand-offs, with dynamic LDS
    and with the observation argument -- appear.  A device whose CU count
    makes one unreachable reports it by name and fails as expected here only."""
    if not _FORMS:   # run alone: the same handles' forms, without their launches
        todo = [(c, n, c.name) for c in ec.CASES for n in (1, c.n)] + \
               [(ec.BY_NAME[name], m, f"{name} n={n}") for name, n in SWEEP for m in (1, n)]
        for c, n, who in todo:
            try:
                tr = trainer_for(c)
            except RuntimeError:   # (its own test reports it)
                continue
            for sc in (1, 0):
                launch_form(tr, n, sc, who)
    for key, nm in FORM_NAMES.items():
        print(f"{nm}: {_FORMS.get(key, 'NOT RUN')}")
    print("worst error / gate per output (error, ref_noise, case, row):")
    for k in ec.OUTPUTS:
        if k in _WORST:
            print(f"  {k}: {_WORST[k][0]:.3f} of its gate ({_WORST[k][1]:.3e}, "
                  f"{_WORST[k][2]:.1e}, {_WORST[k][3]}, {_WORST[k][4]})")
    missing = [nm for key, nm in FORM_NAMES.items() if key not in _FORMS]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if missing and cus != 256:
        pytest.xfail(f"{cus} CUs: forms not reachable: {missing}")
    assert not missing, missing
