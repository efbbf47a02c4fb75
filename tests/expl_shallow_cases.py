"""The one-hidden-layer exploration kernel's cases and their float64
references (test infrastructure, no GPU), modelled on tests/expl_cases.py:
which dimensions, bounds and parameter sets tests/test_gpu_expl_shallow.py runs
through csrc/expl_shallow.hip, the inputs of each, the float64 oracle's
outputs, the fp32 oracle's distance from them (the ``ref_noise`` of
parity.gate) and the quantities of the input conditions
(tests/test_expl_shallow_cases_cpu.py asserts them for every row).

Parameters: fixtures_lib.sac_params(Do, Da, [H], PARAM_SEED, pi_init_w=0.2,
q_init_w=0.1).  Observations and eps are standard normal draws of
RandomState(Do * 1000 + Da * 10 + H); the reference discards its first draw, so
eps_discard is zeros.
"""
import functools

import numpy as np
import torch

from fixtures_lib import sac_params
from oracle import sac_oracle as so

BETA_UB = 4.66
DELTAS = (23.53, 0.5)
PARAM_SEED = 3
N_ROWS = 16
OUTPUTS = ("action", "mu_E", "std", "grad")

# (Do, Da, H)
DIMS = [
    (1, 1, 8),          # minimum dims (lqg width)
    (1, 1, 16),         # the riverswim recipes
    (5, 2, 24),         # H no multiple of 16
    (23, 6, 252),       # H a multiple of 4 only, parts of the gradient of unequal length
    (300, 18, 256),     # Do past one 256-wide block of the row products
    (513, 4, 64),       # one past the observation-argument limit: the host-row single call
    (17, 63, 96),       # Da maximum
    (376, 17, 512),     # Humanoid dims at the widest hidden layer taken
]
EDGE_DIMS = (23, 6, 252)
# rows of one larger draw: a row alone is bitwise the row among N
BATCH_NS = (2, 16, 257)
BATCH_DIMS = (5, 2, 24)


class Case:
    def __init__(self, Do, Da, H, delta=DELTAS[0], edge=None, n=N_ROWS, tag=None):
        self.Do, self.Da, self.H, self.delta, self.edge, self.n = Do, Da, H, delta, edge, n
        dims = f"{Do}x{Da}x{H}"
        self.name = (f"{tag}-" if tag else "") + dims + (f"-{edge}" if edge else "") + f"-d{delta:g}"
        self.draw_key = (tag or "") + dims
        self.seed = Do * 1000 + Da * 10 + H

    @property
    def params_key(self):
        return (self.Do, self.Da, self.H, self.edge)

    def __repr__(self):
        return self.name


def _cases():
    out = []
    for delta in DELTAS:
        for d in DIMS:
            out.append(Case(*d, delta=delta))
        out.append(Case(*EDGE_DIMS, delta=delta, edge="logstd"))
        out.append(Case(*EDGE_DIMS, delta=delta, edge="zeroq"))
    return out


CASES = _cases()
BATCH_CASE = Case(*BATCH_DIMS, n=max(BATCH_NS), tag="batch")
ALL_CASES = CASES + [BATCH_CASE]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


@functools.lru_cache(maxsize=None)
def params_of(key):
    """The case's parameter dicts (fp32 numpy), edge sets applied."""
    Do, Da, H, edge = key
    p = sac_params(Do, Da, [H], PARAM_SEED, pi_init_w=0.2, q_init_w=0.1)
    if edge == "logstd":     # both sides of the log-std clamp [-20, 2]
        b = p["policy"]["last_fc_log_std.bias"]
        b[0::2], b[1::2] = 30.0, -30.0
    elif edge == "zeroq":    # grad == 0: only the + 10e-6 keeps mu_C from 0 / 0
        for q in ("qf1", "qf2"):
            p[q]["last_fc.weight"][:] = 0.0
    else:
        assert edge is None
    return p


@functools.lru_cache(maxsize=None)
def _torch_params(key, dtype):
    p = params_of(key)
    return tuple(so.to_torch_params(p[g], dtype) for g in ("policy", "qf1", "qf2"))


@functools.lru_cache(maxsize=None)
def _draws(seed, n, Do, Da):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, Do)), rs.standard_normal((n, Da)).astype(np.float32)


def inputs(case):
    """(obs float64 [n, Do], eps float32 [n, Da])."""
    return _draws(case.seed, case.n, case.Do, case.Da)


def _oracle(case, dtype):
    obs, eps = inputs(case)
    P, Q1, Q2 = _torch_params(case.params_key, dtype)
    zero = np.zeros(case.Da, np.float32)
    rows = [so.oac_exploration_action(obs[i], P, Q1, Q2, BETA_UB, case.delta, zero, eps[i], dtype=dtype)
            for i in range(case.n)]
    return {k: np.stack([r[k].double().numpy() for r in rows]) for k in OUTPUTS + ("mu_T",)}


def _rel(got, ref):
    n = np.linalg.norm(ref)
    d = np.linalg.norm(got - ref)
    return d if n == 0.0 else d / n


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = BY_NAME[name]
    r64 = _oracle(case, torch.float64)
    r32 = _oracle(case, torch.float32)
    noise = {k: max(_rel(r32[k][i], r64[k][i]) for i in range(case.n)) for k in OUTPUTS}
    for v in r64.values():
        v.setflags(write=False)
    return r64, noise


def reference(case):
    """The float64 oracle's outputs {action, mu_E, std, grad, mu_T: [n, Da]}
    (computed once, read-only)."""
    return _reference(case.name)[0]


def ref_noise(case):
    """{output: the fp32 oracle's largest per-row distance (parity.rel_err)
    from the float64 one} -- parity.gate's ref_noise, never a GPU figure."""
    return _reference(case.name)[1]


def forward64(case):
    """Float64 internals for every row: the policy's layer-0 pre-activations
    [n, H], and per critic (layer-0 pre-activations at a = tanh(mu_T) [n, H], q [n])."""
    obs, _ = inputs(case)
    p = params_of(case.params_key)
    pol = {k: np.asarray(v, np.float64) for k, v in p["policy"].items()}
    pre_p = obs @ pol["fc0.weight"].T + pol["fc0.bias"]
    a = np.tanh(reference(case)["mu_T"])
    x = np.concatenate([obs, a], axis=1)
    critics = []
    for g in ("qf1", "qf2"):
        q = {k: np.asarray(v, np.float64) for k, v in p[g].items()}
        pre0 = x @ q["fc0.weight"].T + q["fc0.bias"]
        critics.append((pre0, (np.maximum(pre0, 0.0) @ q["last_fc.weight"].T + q["last_fc.bias"])[:, 0]))
    return pre_p, critics


def w0_action_rms(case):
    """rms of the critics' layer-0 action columns (the scale of dQ/da)."""
    p = params_of(case.params_key)
    w = np.concatenate([np.asarray(p[g]["fc0.weight"], np.float64)[:, case.Do:].reshape(-1)
                        for g in ("qf1", "qf2")])
    return float(np.sqrt(np.mean(w * w)))
