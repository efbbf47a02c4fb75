"""The network evaluation kernels (csrc/mlp_eval.hip) through the C ABI --
oac_critic_eval, oac_policy_eval, oac_policy_eval_fixed_std called directly on
flat networks built here -- over the shapes their loops can go wrong at: a
hidden width past one 256-thread pass, a width that is no multiple of 64, two
networks with several outputs each, no action input, a row stride wider than
the row, n = 0, up to 63 action dims, and dynamic LDS requests past 64 KiB up
to the 160 KiB the entry points admit.

The reference is float64 torch on the CPU from the same weights (the Jacobian
by autograd, one output at a time).  The gate is parity.gate of an fp32 torch
CPU evaluation's distance from that float64 one; every output whole.

Input condition (not a tolerance): no hidden unit's float64 pre-activation may
lie within 8x the fp32-to-float64 discrepancy of that layer, so no ReLU sign --
which the Jacobian multiplies by -- depends on the summation order.  The seed
that meets it is searched on the CPU (at most 20) and asserted."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF_LOG_2PI = math.log(math.sqrt(2 * math.pi))


# ------------------------------------------------------------ flat networks
def _flat_net(gen, din, H, depth, n_out, out_scale=1.0):
    """(flat fp32 tensor, offsets [w0, b0, w1, b1, wl, bl], dict of the
    tensors): hidden weights N(0, 1/fan_in), biases N(0, 0.1^2)."""
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    t = {"w0": r(H, din) / math.sqrt(din), "b0": 0.1 * r(H)}
    if depth == 2:
        t["w1"], t["b1"] = r(H, H) / math.sqrt(H), 0.1 * r(H)
    t["wl"], t["bl"] = out_scale * r(n_out, H) / math.sqrt(H), 0.1 * r(n_out)
    t = {k: v.float() for k, v in t.items()}
    offs, o = [], 0
    for k in ("w0", "b0", "w1", "b1", "wl", "bl"):
        if k in t:
            offs.append(o)
            o += t[k].numel()
        else:
            offs.append(-1)
    flat = torch.cat([t[k].reshape(-1) for k in ("w0", "b0", "w1", "b1", "wl", "bl") if k in t])
    return flat, offs, t


def _trunk(t, x, dt, pres=None):
    h = x
    for w, b in (("w0", "b0"), ("w1", "b1")):
        if w in t:
            pre = F.linear(h, t[w].to(dt), t[b].to(dt))
            if pres is not None:
                pres.append(pre.detach())
            h = F.relu(pre)
    return h


def _mask_margin(ts, x):
    """Smallest |pre64| / (8 max|pre32 - pre64|) over the hidden layers of the
    networks ``ts`` on the rows ``x`` (> 1: the input condition holds)."""
    worst = np.inf
    for t in ts:
        p32, p64 = [], []
        _trunk(t, x.float(), torch.float32, p32)
        _trunk(t, x.double(), torch.float64, p64)
        for a, b in zip(p32, p64):
            bound = 8.0 * float((a.double() - b).abs().max())
            worst = min(worst, float(b.abs().min()) / max(bound, 1e-300))
    return worst


def _offs(offs):
    return (ctypes.c_int64 * 6)(*offs)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check(got, ref64, ref32, what):
    """Every output whole against float64 under parity.gate of the fp32 CPU
    evaluation's own distance; prints the worst error over its gate."""
    bad, worst = {}, (0.0, None)
    assert sorted(got) == sorted(ref64)
    for k in ref64:
        g = got[k].detach().cpu().numpy()
        assert g.shape == tuple(ref64[k].shape), (k, g.shape, tuple(ref64[k].shape))
        e = parity.rel_err(g, ref64[k].numpy())
        gate = parity.gate(k, parity.rel_err(ref32[k].numpy(), ref64[k].numpy()))
        if e / gate >= worst[0]:
            worst = (e / gate, k)
        if not e <= gate:
            bad[k] = (e, gate)
    print(f"{what}: worst error / gate {worst[0]:.3f} ({worst[1]})")
    assert not bad, (what, bad)


# ------------------------------------------------------------------ critics
def _critic_ref(ts, obs, act, dt, jac):
    x = torch.cat([obs, act], 1).to(dt).requires_grad_(jac)
    q = torch.cat([F.linear(_trunk(t, x, dt), t["wl"].to(dt), t["bl"].to(dt)) for t in ts], 1)
    out = {"q": q.detach()}
    if jac:
        rows = [torch.autograd.grad(q[:, c].sum(), x, retain_graph=True)[0] for c in range(q.shape[1])]
        out["jac"] = torch.stack(rows, 1)   # [N, n_nets Q, din]
    return out


def _critic_inputs(Do, Da, H, depth, Q, n_nets, N):
    """Networks and rows at the first of 20 seeds that meets the input condition."""
    for seed in range(20):
        gen = torch.Generator().manual_seed(1000 + seed)
        nets = [_flat_net(gen, Do + Da, H, depth, Q) for _ in range(n_nets)]
        obs = torch.randn(N, Do, generator=gen)
        act = torch.rand(N, Da, generator=gen) * 2 - 1
        margin = _mask_margin([n[2] for n in nets], torch.cat([obs, act], 1))
        if margin > 1.0:
            return nets, obs, act, seed, margin
    raise AssertionError(f"no seed in 20 meets the mask condition at {(Do, Da, H, depth, Q, n_nets, N)}")


def _run_critic(nets, Do, Da, H, Q, obs_d, ld_obs, act_d, ld_act, N, jac, stream=None):
    from oac_amd import _lib
    L = _lib.lib()
    n = len(nets)
    flats = [f.to(DEV) for f, _, _ in nets]
    q = torch.full((N, n * Q), float("nan"), device=DEV)
    j = torch.full((N, n * Q, Do + Da), float("nan"), device=DEV) if jac else None
    arr = (ctypes.c_void_p * 2)(*[f.data_ptr() for f in flats] + [None] * (2 - n))
    torch.cuda.synchronize()
    sp = _lib.stream_ptr(stream)
    rc = L.oac_critic_eval(arr, n, _offs(nets[0][1]), Do, Da, H, Q, _ptr(obs_d), ld_obs, _ptr(act_d),
                           ld_act, N, _ptr(q), _ptr(j), sp)
    assert rc == 0, L.oac_last_error()
    (stream or torch.cuda.current_stream()).synchronize()
    out = {"q": q}
    if jac:
        out["jac"] = j
    return out


# (Do, Da, H, depth, Q, n_nets, N)
CRITIC_CASES = [
    (1, 1, 4, 1, 1, 1, 1),          # the smallest network
    (5, 2, 24, 1, 1, 2, 37),        # two networks, one layer
    (7, 3, 65, 2, 1, 2, 5),         # one input past a wave
    (9, 4, 48, 2, 3, 2, 4),         # two nets x three outputs: q column and Jacobian index
    (6, 0, 32, 2, 1, 1, 4),         # no action input, act null
    (23, 6, 252, 1, 1, 2, 3),       # H a multiple of 4 only
    (300, 18, 320, 2, 1, 2, 2),     # H and din past 256: second pass of every 256-strided loop
    (376, 17, 256, 2, 10, 1, 3),    # Humanoid dims with ten outputs
]


@pytest.mark.parametrize("jac", [False, True])
@pytest.mark.parametrize("case", CRITIC_CASES)
def test_critic_eval_shapes(case, jac):
    Do, Da, H, depth, Q, n_nets, N = case
    nets, obs, act, seed, margin = _critic_inputs(*case)
    print(f"{case}: seed {seed}, |pre| / b margin {margin:.1f}")
    ts = [n[2] for n in nets]
    got = _run_critic(nets, Do, Da, H, Q, obs.to(DEV), Do, act.to(DEV) if Da else None, Da, N, jac)
    _check(got, _critic_ref(ts, obs, act, torch.float64, jac),
           _critic_ref(ts, obs, act, torch.float32, jac), f"critic {case} jac={jac}")


@pytest.mark.parametrize("jac", [False, True])
def test_critic_eval_reads_columns_of_a_wider_row_buffer(jac):
    """obs and act as columns of one [N, stride] buffer (the replay row):
    ld_obs = ld_act = stride > Do + Da; the other columns hold NaN."""
    case = (9, 4, 48, 2, 3, 2, 4)
    Do, Da, H, depth, Q, n_nets, N = case
    nets, obs, act, _, _ = _critic_inputs(*case)
    stride, o_obs, o_act = 29, 3, 20
    buf = torch.full((N, stride), float("nan"))
    buf[:, o_obs:o_obs + Do], buf[:, o_act:o_act + Da] = obs, act
    buf = buf.to(DEV)
    got = _run_critic(nets, Do, Da, H, Q, buf[:, o_obs:], stride, buf[:, o_act:], stride, N, jac)
    ts = [n[2] for n in nets]
    _check(got, _critic_ref(ts, obs, act, torch.float64, jac),
           _critic_ref(ts, obs, act, torch.float32, jac), f"critic strided jac={jac}")


@pytest.mark.parametrize("jac", [False, True])
def test_critic_eval_on_a_non_default_stream(jac):
    case = (7, 3, 65, 2, 1, 2, 5)
    Do, Da, H, depth, Q, n_nets, N = case
    nets, obs, act, _, _ = _critic_inputs(*case)
    s = torch.cuda.Stream(device=DEV)
    o, a = obs.to(DEV), act.to(DEV)
    torch.cuda.synchronize()
    got = _run_critic(nets, Do, Da, H, Q, o, Do, a, Da, N, jac, stream=s)
    ts = [n[2] for n in nets]
    _check(got, _critic_ref(ts, obs, act, torch.float64, jac),
           _critic_ref(ts, obs, act, torch.float32, jac), f"critic stream jac={jac}")


@pytest.mark.parametrize("jac", [False, True])
def test_critic_eval_of_no_rows_writes_nothing(jac):
    from oac_amd import _lib
    L = _lib.lib()
    Do, Da, H, Q = 5, 2, 24, 1
    nets, obs, act, _, _ = _critic_inputs(Do, Da, H, 1, Q, 2, 3)
    flats = [f.to(DEV) for f, _, _ in nets]
    arr = (ctypes.c_void_p * 2)(*[f.data_ptr() for f in flats])
    q = torch.full((3, 2 * Q), 7.25, device=DEV)
    j = torch.full((3, 2 * Q, Do + Da), 7.25, device=DEV)
    o, a = obs.to(DEV), act.to(DEV)
    rc = L.oac_critic_eval(arr, 2, _offs(nets[0][1]), Do, Da, H, Q, _ptr(o), Do, _ptr(a), Da, 0,
                           _ptr(q), _ptr(j) if jac else None, _lib.stream_ptr())
    assert rc == 0, L.oac_last_error()
    torch.cuda.synchronize()
    assert bool((q == 7.25).all()) and bool((j == 7.25).all())


# ----------------------------------------------------------------- policies
def _policy_ref(t, obs, eps, dt, fixed_std=None):
    """The six outputs of TanhGaussianPolicy.forward in ``dt``; the head is
    stacked [2 Da, H], mean rows first.  eps None: deterministic."""
    h = _trunk(t, obs.to(dt), dt)
    hd = F.linear(h, t["wl"].to(dt), t["bl"].to(dt))
    Da = hd.shape[1] // 2
    mean = hd[:, :Da]
    if fixed_std is None:
        log_std = torch.clamp(hd[:, Da:], -20.0, 2.0)
        std = torch.exp(log_std)
    else:
        std = fixed_std.to(dt)[None].expand_as(mean)
        log_std = torch.log(std)
    if eps is None:
        z, lp = mean, torch.zeros(mean.shape[0], dtype=dt)
    else:
        z = mean + std * eps.to(dt)
        a = torch.tanh(z)
        lp = (-(z - mean) ** 2 / (2 * std * std) - torch.log(std) - HALF_LOG_2PI
              - torch.log(1 - a * a + 1e-6)).sum(1)
    return dict(action=torch.tanh(z), mean=mean.clone(), log_std=log_std.clone(), log_prob=lp,
                std=std.clone(), pre_tanh=z.clone())


def _policy_inputs(Do, Da, H, depth, N, ls_scale=0.05, ls_bias=-1.0):
    """A flat policy (small heads: |tanh z| < 0.999), rows and eps at the first
    of 20 seeds that meets the input condition."""
    for seed in range(20):
        gen = torch.Generator().manual_seed(2000 + seed)
        flat, offs, t = _flat_net(gen, Do, H, depth, 2 * Da, out_scale=0.3)
        t["wl"][Da:] *= ls_scale / 0.3
        t["bl"][Da:] = ls_bias + 0.05 * torch.randn(Da, generator=gen)
        flat = torch.cat([t[k].reshape(-1) for k in ("w0", "b0", "w1", "b1", "wl", "bl") if k in t])
        obs = torch.randn(N, Do, generator=gen)
        eps = 0.5 * torch.randn(N, Da, generator=gen)
        margin = _mask_margin([t], obs)
        if margin > 1.0:
            return (flat, offs, t), obs, eps, seed, margin
    raise AssertionError(f"no seed in 20 meets the mask condition at {(Do, Da, H, depth, N)}")


def _run_policy(net, Do, Da, H, obs, eps, want_lp, N, fixed_std=None):
    from oac_amd import _lib
    L = _lib.lib()
    flat, offs, _ = net
    flat, o = flat.to(DEV), obs.to(DEV)
    e = None if eps is None else eps.to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = dict(action=nan(N, Da), mean=nan(N, Da), log_std=nan(N, Da), std=nan(N, Da),
               pre_tanh=nan(N, Da))
    lp = nan(N) if want_lp else None
    tail = (_ptr(e), _ptr(out["action"]), _ptr(out["mean"]), _ptr(out["log_std"]), _ptr(lp),
            _ptr(out["std"]), _ptr(out["pre_tanh"]), _lib.stream_ptr())
    if fixed_std is None:
        rc = L.oac_policy_eval(_ptr(flat), _offs(offs), Do, Da, H, _ptr(o), Do, N, *tail)
    else:
        sd = fixed_std.to(DEV)
        rc = L.oac_policy_eval_fixed_std(_ptr(flat), _offs(offs), Do, Da, H, _ptr(o), Do, N, _ptr(sd),
                                         *tail)
    assert rc == 0, L.oac_last_error()
    torch.cuda.synchronize()
    if want_lp:
        out["log_prob"] = lp
    return out


def _drop_lp(ref, want_lp):
    return ref if want_lp else {k: v for k, v in ref.items() if k != "log_prob"}


# (Do, Da, H, depth, N)
POLICY_CASES = [(1, 1, 4, 1, 1), (5, 2, 24, 1, 37), (17, 63, 96, 1, 3), (300, 18, 320, 2, 2),
                (376, 17, 256, 2, 5)]


@pytest.mark.parametrize("want_lp", [False, True])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("case", POLICY_CASES)
def test_policy_eval_shapes(case, sampled, want_lp):
    Do, Da, H, depth, N = case
    net, obs, eps, seed, margin = _policy_inputs(*case)
    eps = eps if sampled else None
    r64 = _policy_ref(net[2], obs, eps, torch.float64)
    assert float(r64["action"].abs().max()) < 0.999   # (log(1 - a^2 + 1e-6) amplifies nothing)
    print(f"{case}: seed {seed}, |pre| / b margin {margin:.1f}")
    got = _run_policy(net, Do, Da, H, obs, eps, want_lp, N)
    _check(got, _drop_lp(r64, want_lp), _drop_lp(_policy_ref(net[2], obs, eps, torch.float32), want_lp),
           f"policy {case} sampled={sampled} log_prob={want_lp}")
    if not sampled and want_lp:
        assert not got["log_prob"].any()


@pytest.mark.parametrize("want_lp", [False, True])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("case", POLICY_CASES)
def test_policy_eval_fixed_std_shapes(case, sampled, want_lp):
    """A per-dimension std vector: log_std = log(std), unclamped; the log-prob
    is summed in double on the device."""
    Do, Da, H, depth, N = case
    net, obs, eps, seed, margin = _policy_inputs(*case)
    eps = eps if sampled else None
    std = 0.1 + 0.4 * torch.rand(Da, generator=torch.Generator().manual_seed(5))
    r64 = _policy_ref(net[2], obs, eps, torch.float64, fixed_std=std)
    assert float(r64["action"].abs().max()) < 0.999
    assert torch.equal(r64["log_std"][0], torch.log(std.double()))
    got = _run_policy(net, Do, Da, H, obs, eps, want_lp, N, fixed_std=std)
    _check(got, _drop_lp(r64, want_lp),
           _drop_lp(_policy_ref(net[2], obs, eps, torch.float32, fixed_std=std), want_lp),
           f"policy fixed std {case} sampled={sampled} log_prob={want_lp}")


@pytest.mark.parametrize("sampled", [False, True])
def test_policy_eval_clamps_the_log_std_at_both_ends(sampled):
    """The log-std head's weights scaled to 40 / sqrt(H) around a bias of -9:
    raw values past -20, past 2 and between them.  With eps the log-prob is not requested: at std = e^-20 the term
    (z - mean)^2 / (2 std^2) is the rounding of z = mean + std eps against a
    std of 2e-9, which no fp32 evaluation determines, and at std = e^2 the
    tanh saturates; the five other outputs are well conditioned and checked
    whole.  Deterministic: log_prob requested, all zeros."""
    Do, Da, H, depth, N = 5, 2, 24, 1, 37
    net, obs, eps, _, _ = _policy_inputs(Do, Da, H, depth, N, ls_scale=40.0, ls_bias=-9.0)
    eps = eps if sampled else None
    r64 = _policy_ref(net[2], obs, eps, torch.float64)
    assert bool((r64["log_std"] == -20.0).any()) and bool((r64["log_std"] == 2.0).any())
    assert bool(((r64["log_std"] > -20.0) & (r64["log_std"] < 2.0)).any())
    want_lp = not sampled
    got = _run_policy(net, Do, Da, H, obs, eps, want_lp, N)
    _check(got, _drop_lp(r64, want_lp), _drop_lp(_policy_ref(net[2], obs, eps, torch.float32), want_lp),
           f"policy clamps sampled={sampled}")
    ls = got["log_std"].cpu()
    assert float(ls.min()) == -20.0 and float(ls.max()) == 2.0


# ---------------------------------------------------------- LDS past 64 KiB
def test_critic_eval_with_dynamic_lds_past_64_kib():
    """One-layer critics whose workgroup requests (din + 4 H + Q + 4) floats of
    dynamic LDS: (3, 1, 4100) asks 65,636 B, the smallest request past 64 KiB;
    (10, 1, 10236) asks 163,840 B, the largest the entry point admits.  The
    runtime takes both launches as they are (no hipFuncSetAttribute call in
    csrc/): outputs and Jacobian match float64 like every other case."""
    jac = True
    for Do, Da, H in ((3, 1, 4100), (10, 1, 10236)):
        assert 4 * (Do + Da + 4 * H + 1 + 4) == {4100: 65636, 10236: 160 * 1024}[H]
        case = (Do, Da, H, 1, 1, 1, 2)
        nets, obs, act, seed, margin = _critic_inputs(*case)
        print(f"{case}: seed {seed}, |pre| / b margin {margin:.1f}")
        ts = [n[2] for n in nets]
        got = _run_critic(nets, Do, Da, H, 1, obs.to(DEV), Do, act.to(DEV), Da, 2, jac)
        _check(got, _critic_ref(ts, obs, act, torch.float64, jac),
               _critic_ref(ts, obs, act, torch.float32, jac), f"critic LDS {case} jac={jac}")
