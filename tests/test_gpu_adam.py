"""oac_adam_polyak, the stand-alone optimizer entry point (bench.py times it,
no plan test calls it), against a float64 restatement of torch-1.4 Adam +
Polyak as csrc/adam_common.h states them:

    m = b1 m + (1 - b1) g          v = b2 v + (1 - b2) g^2
    p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),  bc_i = 1 - b_i^t
    target = (1 - tau) target + tau p    (post-step p; when n_steps % period == 0)

with the advance semantics of include/oac_amd.h: advance = 0 takes
t = n_steps + 1 and snapshots n_steps; advance = 1 takes t from the snapshot,
then n_steps = snapshot + 1 and batch_counter += 1.

Five consecutive steps (t = 1..5) from a zeroed step state, each an advance=0
call on one range (with a target) then an advance=1 call on another (without):
the critic-then-policy order of a real step.  Gradients have |g| in [0.1, 1]
(nothing in Adam's sign band, parity.py module doc).

Gate per tensor: parity.gate(key, ref_noise), ref_noise = the distance of a
numpy float32 restatement from the float64 one after the same five steps.
Measured on MI355X (all sizes, both periods): m and v equal the float32
restatement bit for bit, p and target to within 4.3e-9 relative; errors
against float64 at most p 6.3e-8, m 1.0e-7, v 1.7e-7, target 1.3e-7 -- the
gate is 1e-5 throughout (ref_noise at most 1.7e-7)."""
import ctypes

import numpy as np
import pytest
import torch

import parity

pytestmark = pytest.mark.gpu

# lr and tau far above the trainers' (3e-4, 5e-3) so that every term is
# visible at the 1e-5 gate: a Polyak on the pre-step p moves the target by
# tau * lr per step -- 1.5e-6 there, 2.5e-3 here
LR, B1, B2, EPS, TAU = 1e-2, 0.9, 0.999, 1e-8, 0.25
STEPS = 5


class _Range:
    """One flat parameter range: p, m, v (+ target) and its numpy twins in
    ``dt`` (float64: the oracle; float32: the reference's own rounding)."""

    def __init__(self, n, rs, with_target):
        self.n = n
        self.init = dict(p=rs.standard_normal(n).astype(np.float32),
                         m=(0.1 * rs.standard_normal(n)).astype(np.float32),
                         v=(0.01 * rs.random_sample(n)).astype(np.float32))   # v >= 0
        if with_target:
            self.init["target"] = rs.standard_normal(n).astype(np.float32)

    def state(self, dt):
        return {k: x.astype(dt) for k, x in self.init.items()}

    def device(self):
        return {k: torch.from_numpy(x.copy()).cuda() for k, x in self.init.items()}


def _grad(rs, n):
    return (rs.uniform(0.1, 1.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)


def _ref_step(s, g, t, polyak, dt):
    """One Adam (+ Polyak) step at bias-correction step t in dtype dt; the
    step size and sqrt(bc2) are formed in double and rounded to dt, as
    torch-1.4 forms them in Python floats."""
    f = dt
    g = g.astype(dt)
    bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    s["m"] = s["m"] * f(B1) + f(1.0 - B1) * g
    s["v"] = s["v"] * f(B2) + (f(1.0 - B2) * g) * g
    denom = np.sqrt(s["v"]) / f(np.sqrt(bc2)) + f(EPS)
    s["p"] = s["p"] + (-f(LR / bc1) * s["m"]) / denom
    if polyak and "target" in s:
        s["target"] = s["target"] * f(1.0 - float(np.float32(TAU))) + s["p"] * f(np.float32(TAU))


def _call(L, d, g, n, period, state, advance):
    return L.oac_adam_polyak(d["p"].data_ptr(), g.data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(),
                             n, d["target"].data_ptr() if "target" in d else None, TAU, period,
                             LR, B1, B2, EPS, state.data_ptr(), advance,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


# 4: one float4; 1020: a partial last block; 2,097,156 > 2048 blocks x 256
# threads x 4 floats: the grid-stride loop's second pass (one float4 of it)
@pytest.mark.parametrize("period", [1, 2])
@pytest.mark.parametrize("n", [4, 1020, 2_097_156])
def test_adam_polyak_against_float64(n, period):
    from oac_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(n % 1000 + period)
    n2 = 1020 if n != 1020 else 260          # the advance=1 range (no target)
    ra, rb = _Range(n, rs, True), _Range(n2, rs, False)
    da, db = ra.device(), rb.device()
    r64, r32 = (ra.state(np.float64), rb.state(np.float64)), (ra.state(np.float32), rb.state(np.float32))
    state = torch.zeros(8, dtype=torch.int64, device="cuda")   # a zeroed 64-byte StepState

    def words():
        w = state.cpu().numpy()
        return int(w[0]), int(w[1]), int(w[3])   # n_steps, batch_counter, t_snapshot

    for k in range(STEPS):
        t = k + 1
        ga, gb = _grad(rs, n), _grad(rs, n2)
        polyak = k % period == 0
        _lib.check(_call(L, da, torch.from_numpy(ga).cuda(), n, period, state, 0))
        assert words() == (k, k, k), "advance=0 snapshots n_steps and advances nothing"
        _lib.check(_call(L, db, torch.from_numpy(gb).cuda(), n2, period, state, 1))
        assert words() == (k + 1, k + 1, k), "advance=1: n_steps = snapshot + 1, batch_counter += 1"
        for r, dt in ((r64, np.float64), (r32, np.float32)):
            _ref_step(r[0], ga, t, polyak, dt)
            _ref_step(r[1], gb, t, polyak, dt)
    torch.cuda.synchronize()
    errs, bad = {}, {}
    for tag, d, w64, w32 in (("a", da, r64[0], r32[0]), ("b", db, r64[1], r32[1])):
        for key in w64:
            got = d[key].cpu().numpy()
            assert np.isfinite(got).all()
            ref_noise = parity.rel_err(w32[key], w64[key])
            e = parity.rel_err(got, w64[key])
            tol = parity.gate(f"{tag}/{key}", ref_noise)
            errs[f"{tag}/{key}"] = (e, tol, ref_noise, parity.rel_err(got, w32[key]))
            if not e <= tol:
                bad[f"{tag}/{key}"] = errs[f"{tag}/{key}"]
    print(f"adam n={n} period={period} (error, gate, ref_noise, vs float32): " +
          ", ".join(f"{k} {v[0]:.2e}/{v[1]:.0e}/{v[2]:.2e}/{v[3]:.2e}" for k, v in errs.items()))
    assert not bad, f"(error, gate, ref_noise, vs float32) {bad}; all: {errs}"
    # the target moved on the Polyak steps only, and only where there is one
    assert not np.array_equal(da["target"].cpu().numpy(), ra.init["target"])


def test_adam_polyak_skips_polyak_off_period():
    """period = 2 at n_steps = 1: Adam runs, the target is left alone."""
    from oac_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(0)
    r = _Range(1020, rs, True)
    d = r.device()
    state = torch.zeros(8, dtype=torch.int64, device="cuda")
    state[0] = 1
    _lib.check(_call(L, d, torch.from_numpy(_grad(rs, 1020)).cuda(), 1020, 2, state, 0))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d["target"].cpu().numpy(), r.init["target"])
    assert not np.array_equal(d["p"].cpu().numpy(), r.init["p"])


def test_adam_polyak_rejects_a_ragged_range():
    """n = 6 (not a 16-byte multiple): nonzero with a message, nothing launched."""
    from oac_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(1)
    r = _Range(8, rs, True)
    d = r.device()
    state = torch.zeros(8, dtype=torch.int64, device="cuda")
    state[0] = 3
    g = torch.from_numpy(_grad(rs, 8)).cuda()
    for advance in (0, 1):
        rc = _call(L, d, g, 6, 1, state, advance)
        assert rc != 0
        assert L.oac_last_error().decode(errors="replace").strip()
    torch.cuda.synchronize()
    for k, x in r.init.items():
        np.testing.assert_array_equal(d[k].cpu().numpy(), x)
    assert state.cpu().numpy().tolist() == [3, 0, 0, 0, 0, 0, 0, 0]
