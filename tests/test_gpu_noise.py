"""The device noise itself.  Every parity test feeds the step its eps; training
draws them on the device (OAC_STEP_DEVICE_EPS, the eps-free exploration call)
from csrc/kernels.h philox_normal, called from six sites with their own
indexing:

  A   replay.hip gather_kernel      eps waves after the gather rows
  B   gemm_small.hip side blocks    the small-batch drop-in step's layer-0 launch
  C   gemm_fwd.hip side blocks      the large-batch drop-in step, 256 x 256 grid-stride
  D   expl_split.hip                tagged single observation, batched rows, twin kernel

Each drawn value is compared here with oracle/philox_oracle.py (Philox4x32-10
from the published algorithm, checked on the CPU by tests/test_philox_oracle.py)
at the seed, counter, stream and element index the noise contract states
(DESIGN.md "Noise contract").

Tolerance: noise = max |oracle in float32 - oracle in float64| over the same
elements (the restatement's own rounding, 8e-7 .. 1e-6 here); a device value
may be 4 x noise from the float64 oracle (device logf / sinf / cosf a couple
of ulp from numpy's).  A wrong bit anywhere in the counter layout moves values
by O(1).  Measured on MI355X, worst device-to-oracle distance per site against
its 4 x noise allowance: A 7.8e-7 / 2.7e-6, B 8.9e-7 / 3.2e-6, C 9.3e-7 /
3.7e-6 (the particle plan's sites the same figures); at most 1.5 x noise
anywhere.  Exploration (D): actions at most 0.22 of their allowance.

With n_eps = 1 the noise is the rounding of that one element, not a maximum
over many: the allowance is 3.9e-8 .. 2.1e-6 at the counters tested (device
distances 9.9e-9 .. 5.1e-7).  It is an estimate from a single sample there:
at seed 2^32 + 11, counter 2^32 + 3 the two restatements agree to 6.0e-9 while
the device value is one float32 ulp (1.1e-7) from them."""
import numpy as np
import pytest
import torch

import parity
from fixtures_lib import sac_params, synthetic_transitions
from gpu_helpers import Space, producers, sac_trainer_for
from oracle.philox_oracle import philox_normal

pytestmark = pytest.mark.gpu

BIG_SEED = 2 ** 32 + 11   # the key's high word


# ------------------------------------------------------------- step draws
def _sac(Do, Da, H, seed):
    from oac_amd import SACTrainer
    pp, qp = producers(sac_params(Do, Da, [H, H], 3, pi_init_w=0.2, q_init_w=0.1))
    return SACTrainer(pp, qp, action_space=Space(Da), policy_lr=3e-4, qf_lr=3e-4,
                      soft_target_tau=5e-3, use_automatic_entropy_tuning=True, seed=seed)


def _particle(Do, Da, H, seed, K=7):
    from oac_amd import ParticleTrainerOAC
    params = sac_params(Do, Da, [H, H], 3, q_out=K, pi_init_w=0.2, q_init_w=0.1,
                        q_last_bias=np.linspace(0.0, 30.0, K))
    pp, qp = producers(params, q_keys=("qf1", "qf2", "target_qf1", "target_qf2", "qf1",
                                       "target_qf1"))
    return ParticleTrainerOAC(pp, qp, n_estimators=K, action_space=Space(Da), policy_lr=3e-4,
                              qf_lr=3e-4, soft_target_tau=5e-3, use_automatic_entropy_tuning=True,
                              deterministic=False, q_min=0.0, q_max=30.0, share_layers=True,
                              seed=seed)


def _host_batch(Do, Da, B, seed):
    data = synthetic_transitions(max(4 * B, 64), Do, Da, seed=seed)
    idx = np.random.RandomState(seed).randint(0, len(data["rewards"]), B)
    return {k: v[idx] for k, v in data.items()}


def _replay(Do, Da, **kw):
    from oac_amd import ReplayBuffer
    rb = ReplayBuffer(2000, Space(Do), Space(Da), device="cuda:0", **kw)
    d = synthetic_transitions(2000, Do, Da, seed=1)
    rb.load_transitions(torch.from_numpy(rb._rows_from(
        d["observations"], d["actions"], d["rewards"], d["next_observations"],
        d["terminals"])).cuda())
    return rb


def _check_draws(tr, plan, counter, B, Da, what):
    """eps1 / eps2 of the step just run against the oracle at ``counter``:
    the figures are printed, the misses returned (asserted by the caller
    after both steps, so a miss at the first does not hide the second's)."""
    got = {s: plan.views[f"eps{s}"].cpu().numpy().astype(np.float64) for s in (1, 2)}
    idx = np.arange(B * Da)
    misses = []
    for s in (1, 2):
        assert got[s].shape == (B, Da)
        assert not np.isnan(got[s]).any(), \
            f"{what}: eps{s} has {int(np.isnan(got[s]).sum())} unwritten elements"
        ref = philox_normal(tr.seed, counter, s, idx, np.float64)
        noise = np.abs(philox_normal(tr.seed, counter, s, idx, np.float32).astype(np.float64)
                       - ref).max()
        d = np.abs(got[s].reshape(-1) - ref)
        print(f"{what} counter={counter} eps{s}: device-oracle {d.max():.3e}, noise {noise:.3e}, "
              f"allowance {4 * noise:.3e}")
        if not d.max() <= 4 * noise:
            misses.append(f"{what}: eps{s} at counter {counter} is {d.max():.3e} from the oracle "
                          f"(allowance 4 x {noise:.3e}); first bad element "
                          f"{int(np.argmax(d > 4 * noise))}")
    assert not np.array_equal(got[1], got[2]), f"{what}: streams 1 and 2 are equal"
    return misses


def _two_steps(tr, B, Da, step, want_bits, what):
    """Two consecutive steps, each with NaN-filled eps views before it:
    ``step()`` -> the plan it ran on (the plan's views are filled by
    ``step(fill)`` through the callback it is given before the launch)."""
    from oac_amd._lib import TRACE, lib
    misses = []
    for k in range(2):
        c0 = int(tr.step_state[1].item())

        def fill(plan):
            for s in (1, 2):
                plan.views[f"eps{s}"].fill_(float("nan"))
        plan = step(fill)
        torch.cuda.synchronize()
        assert plan is tr._last_plan
        assert int(tr.step_state[1].item()) == c0 + 1, "the batch counter advances by 1 per step"
        bits = lib().oac_sac_trace(plan.handle, 1)
        for name, on in want_bits.items():
            assert bool(bits & TRACE[name]) == on, \
                f"{what}: trace bit {name} = {bool(bits & TRACE[name])} (bits {bits}): another site ran"
        misses += _check_draws(tr, plan, c0, B, Da, f"{what} step {k}")
    assert not misses, misses


# (Do, Da, H, B, seed, first counter): n_eps = 1 is half a Box-Muller pair;
# n_eps = 185 a partial last wave with pairs straddling rows (odd Da), from a
# fresh trainer and from a counter above 2^32 (the counter's high word)
@pytest.mark.parametrize("Do,Da,H,B,seed,c_start", [(11, 1, 32, 1, BIG_SEED, 0),
                                                    (7, 5, 48, 37, 7, 0),
                                                    (7, 5, 48, 37, 7, 2 ** 32 + 3)])
def test_gather_launch_eps_only(Do, Da, H, B, seed, c_start):
    """Site A without gather rows: train_from_torch(batch), the launch is eps
    waves only."""
    tr = _sac(Do, Da, H, seed)
    tr.step_state[1] = c_start
    batch = _host_batch(Do, Da, B, 1)

    def step(fill):
        plan = tr._plan(B)
        fill(plan)
        tr.train_from_torch(batch)
        return plan
    _two_steps(tr, B, Da, step, dict(direct=False, direct_big=False), "A (eps only)")


def test_gather_launch_eps_after_rows():
    """Site A behind gather rows (37 rows: the eps waves start at the padded
    workgroup boundary 48): a device-index batch through train_device_batch."""
    Do, Da, H, B = 7, 5, 48, 37
    tr = _sac(Do, Da, H, BIG_SEED)
    rb = _replay(Do, Da, index_source="device", seed=4)
    tr.train(rb.random_batch(B))   # (creates the plan of this path)
    plan0 = tr._last_plan

    def step(fill):
        fill(plan0)
        tr.train(rb.random_batch(B))
        return plan0
    _two_steps(tr, B, Da, step, dict(direct=False, direct_big=False), "A (after rows)")


def _dropin(make, Do, Da, H, B, seed, want_bits, what):
    tr = make(Do, Da, H, seed)
    rb = _replay(Do, Da)
    np.random.seed(5)

    def step(fill):
        batch = rb.random_batch(B)
        plan = tr._dropin_plan(batch)
        fill(plan)
        tr.train(batch)
        return plan
    _two_steps(tr, B, Da, step, want_bits, what)


# 37 x 5: fewer eps than one pass of the side blocks; 1000 x 17 = 17,000: several
# passes of the stride loop (125 side workgroups)
@pytest.mark.parametrize("Do,Da,H,B,seed", [(7, 5, 48, 37, BIG_SEED), (11, 17, 64, 1000, 7)])
def test_small_batch_dropin_side_blocks(Do, Da, H, B, seed):
    """Site B: rb.random_batch(B) + tr.train(batch) below 1024 rows."""
    _dropin(_sac, Do, Da, H, B, seed, dict(direct=True, direct_big=False), "B")


# 1029 x 6: ragged; 4096 x 17 = 69,632 > 256 x 256: the grid-stride loop's second pass
@pytest.mark.parametrize("Do,Da,H,B,seed", [(13, 6, 64, 1029, 7), (11, 17, 64, 4096, BIG_SEED)])
def test_large_batch_dropin_side_blocks(Do, Da, H, B, seed):
    """Site C: the same call at >= 1024 rows."""
    _dropin(_sac, Do, Da, H, B, seed, dict(direct=False, direct_big=True), "C")


@pytest.mark.parametrize("Do,Da,H,B,seed,big", [(7, 5, 48, 37, 7, False),
                                                (11, 17, 64, 4096, BIG_SEED, True)])
def test_particle_dropin(Do, Da, H, B, seed, big):
    """ParticleTrainerOAC (deterministic=False) wires its own eps
    (particle_plan.hip): the gather launch behind its rows at small batch
    (site A; this kind has no small-batch direct step), side blocks of the
    layer-0 launch at large batch (site C)."""
    _dropin(_particle, Do, Da, H, B, seed, dict(direct=False, direct_big=big),
            "particle C" if big else "particle A (after rows)")


# ------------------------------------------------------------ exploration
def _expl_trainer(name, seed):
    meta, g = parity.load(name)
    if "K" not in meta:
        params = sac_params(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["seed"],
                            pi_init_w=meta["pi_init_w"], q_init_w=meta["q_init_w"])
        m = dict(obs_dim=meta["obs_dim"], act_dim=meta["act_dim"], hidden=meta["hidden"],
                 discount=0.99, reward_scale=1.0, lr=3e-4, tau=5e-3, auto_alpha=True,
                 log_alpha0=0.0, seed=meta["seed"], pi_init_w=meta["pi_init_w"],
                 q_init_w=meta["q_init_w"])
        tr = sac_trainer_for(m, params=params, seed=seed)
        share = False
    else:
        from oac_amd import ParticleTrainerOAC
        K = meta["K"]
        params = sac_params(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["seed"],
                            pi_init_w=meta["pi_init_w"], q_init_w=meta["q_init_w"], q_out=K,
                            q_last_bias=np.linspace(0.0, 50.0, K))
        pp, qp = producers(params, q_keys=("qf1", "qf2", "target_qf1", "target_qf2", "qf1",
                                           "target_qf1"))
        tr = ParticleTrainerOAC(pp, qp, n_estimators=K, action_space=Space(meta["act_dim"]),
                                deterministic=False, q_min=0.0, q_max=50.0, share_layers=True,
                                seed=seed)
        share = True
    hp = dict(beta_UB=meta["beta_UB"], delta=meta["delta"], share_layers=share)
    return meta, g, tr, hp


def _expl_case(tr, hp, obs, c_start):
    """One eps-free call on ``obs`` [n, Do] against the same call fed the
    oracle's float32 draws (handle seed tr.seed + 1, stream 3, the call's
    counter, element r * Da + t)."""
    from oac_amd import get_optimistic_exploration_action, get_optimistic_exploration_actions
    n, Da = obs.shape[0], tr.act_dim
    kw = dict(policy=tr.policy, qfs=tr.qfs, hyper_params=hp)
    tr.step_state[2] = c_start
    c0 = int(tr.step_state[2].item())
    if n == 1:   # the per-environment-step call: observation in the arguments, tagged granules
        a, info = get_optimistic_exploration_action(obs[0], **kw)
        assert info == {}
        out = tr._expl_handle(1).out_np   # the call's unpacked [action | mu_E | std]
        np.testing.assert_array_equal(out[0, 0], a)
        free = dict(a=a[None, :], mu_E=out[1].copy(), std=out[2].copy())
    else:
        A, info = get_optimistic_exploration_actions(obs, return_info=True, **kw)
        free = dict(a=A, mu_E=info["mu_E"], std=info["std"])
    assert int(tr.step_state[2].item()) == c0 + 1, "one counter value per eps-free call"
    idx = np.arange(n * Da)
    e32 = philox_normal(tr.seed + 1, c0, 3, idx, np.float32)
    noise = np.abs(e32.astype(np.float64)
                   - philox_normal(tr.seed + 1, c0, 3, idx, np.float64)).max()
    tr.step_state[2] = c0
    if n == 1:
        a, info = get_optimistic_exploration_action(obs[0], eps=e32, return_info=True, **kw)
        fed = dict(a=a[None, :], mu_E=info["mu_E"][None, :], std=info["std"][None, :])
    else:
        A, info = get_optimistic_exploration_actions(obs, eps=e32.reshape(n, Da),
                                                     return_info=True, **kw)
        fed = dict(a=A, mu_E=info["mu_E"], std=info["std"])
    assert np.isfinite(free["a"]).all() and np.isfinite(fed["a"]).all()
    np.testing.assert_array_equal(free["mu_E"], fed["mu_E"])
    np.testing.assert_array_equal(free["std"], fed["std"])
    # tanh is 1-Lipschitz: |da| <= std |d eps|; 2^-21 = two float32 ulps at
    # |z| < 8 for the roundings of ev * sd + mu_E and of tanhf
    allow = fed["std"].astype(np.float64) * (4 * noise) + 2.0 ** -21
    d = np.abs(free["a"].astype(np.float64) - fed["a"].astype(np.float64))
    ratio = float((d / allow).max())
    print(f"exploration n={n} counter={c0}: max |a_free - a_fed| {d.max():.3e}, "
          f"{ratio:.3f} of the allowance (noise {noise:.3e})")
    assert (d <= allow).all(), (f"n={n}: action {d.max():.3e} from the fed-eps call, "
                                f"{ratio:.1f} x the allowance; first bad row "
                                f"{int(np.argmax((d > allow).any(axis=1)))}")
    return free


@pytest.mark.parametrize("name,seed", [("oac_expl_small", 9), ("oac_expl_shared_small", BIG_SEED)])
def test_exploration_draws(name, seed):
    """Twin critics and one shared-layer critic with K heads (both exploration
    kernels): n = 1 (tagged path), 5, and 300 -- two launches of one call,
    which must share one counter and index rows globally."""
    meta, g, tr, hp = _expl_trainer(name, seed)
    rs = np.random.RandomState(1)
    obs = np.concatenate([g["obs"], rs.standard_normal((300, meta["obs_dim"]))])[:300]
    _expl_case(tr, hp, obs[:1], 0)
    _expl_case(tr, hp, obs[:1], 2 ** 32 + 1)     # the counter's high word; the same handle again
    _expl_case(tr, hp, obs[:5], 4)
    free = _expl_case(tr, hp, obs, 5)
    assert not np.array_equal(free["a"][0], free["a"][256])
    # row 256 (first of the second launch) with row 0's observation: still its own draw
    obs2 = obs.copy()
    obs2[256] = obs2[0]
    free = _expl_case(tr, hp, obs2, 6)
    np.testing.assert_array_equal(free["mu_E"][0], free["mu_E"][256])
    assert not np.array_equal(free["a"][0], free["a"][256]), "row 256 drew row 0's eps"


def test_exploration_draws_humanoid_single():
    """n = 1 at the Humanoid shape (Do = 376 in the kernel arguments, Da = 17)."""
    meta, g, tr, hp = _expl_trainer("oac_expl_humanoid", 3)
    _expl_case(tr, hp, g["obs"][:1], 0)
    _expl_case(tr, hp, g["obs"][1:2], 1)
