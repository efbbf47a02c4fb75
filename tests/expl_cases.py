"""The exploration kernels' shape-edge cases and their float64 references
(test infrastructure, no GPU): which dimensions, bounds and parameter sets
tests/test_gpu_expl_shapes.py runs through csrc/expl_split.hip, the inputs of
each, the float64 oracle's outputs, the fp32 oracle's distance from them (the
``ref_noise`` of parity.gate) and the input conditions under which the
comparison is well defined (tests/test_expl_cases_cpu.py asserts them for
every row).

Parameters: fixtures_lib.sac_params(Do, Da, [H, H], PARAM_SEED, q_out,
pi_init_w=0.2, q_init_w=0.1); the K-head critics take the last bias
linspace(0, 50, K).  Observations and eps are standard normal draws of
RandomState(case.seed); the reference discards its first draw, so eps_discard
is zeros.
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
UB_TRAINER_DELTA = 0.5          # ParticleTrainerOAC(delta=...): a delta_index inside (0, K-1) for K > 2
OUTPUTS = ("action", "mu_E", "std", "grad")

# (Do, Da, H): twin critics (SACTrainer)
TWIN_DIMS = [
    (1, 1, 8),          # minimum dims, fewer rows than parts
    (5, 2, 40),         # H no multiple of 16
    (23, 6, 250),       # H just under the twin limit, no multiple of 4
    (300, 18, 256),     # 2*H*Da == 9216: the last shape the twin kernel takes; second k pass
    (300, 19, 256),     # first past the twin budget: split kernel, twin critics
    (512, 4, 64),       # observation-argument limit
    (513, 4, 64),       # one past it: split kernel, host-row single call
    (29, 32, 64),       # twin Da limit
    (29, 33, 64),       # one past it: split kernel
    (17, 63, 96),       # Da maximum
    (111, 8, 257),      # H one past the twin limit
    (111, 8, 320),      # a common wider layer_size
    (376, 17, 512),     # Humanoid with 512 units
]
# the twin shapes oac_expl_twin_kernel takes; every other one (and every K-head
# shape) runs oac_expl_split_kernel
TWIN_KERNEL_DIMS = {(1, 1, 8), (5, 2, 40), (23, 6, 250), (300, 18, 256), (512, 4, 64), (29, 32, 64)}
# (Do, Da, H, K): one shared-layer critic with K heads (ParticleTrainerOAC)
HEAD_DIMS = [(7, 5, 48, 2), (13, 6, 80, 16), (23, 6, 250, 7), (376, 17, 512, 10)]
EDGE_TWIN = (23, 6, 250)
EDGE_HEADS = (13, 6, 80, 16)
# the group-size sweep: rows of one 257-row draw per shape
SWEEP_NS = (2, 9, 12, 42, 85, 128, 129, 257)
SWEEP_DIMS = [(23, 6, 250, None), (300, 19, 256, None), (23, 6, 250, 7)]
# Beyond the issue's table: twin critics wide enough that a split-kernel
# workgroup owning two of the 32 column parts holds more dh1 columns than 2H /
# G + 32 (from 2H = 1196 at G = 28, 2H = 1195 at G = 15: 9 and 17 observations
# on 256 CUs)
WIDE_DIMS = (5, 2, 640, None)
WIDE_NS = (9, 17)

# a case whose draw violates an input condition gets another seed here (no row
# is ever left out): name -> seed
# The 257-row sweep draws hold ~250k critic pre-activations each, so a draw
# with none within 5e-6 rms of 0 is the exception: these are the first seeds
# (default + j * 100000) whose draw keeps every one 2e-5 rms away.
SEED_OVERRIDES = {
    "sweep23x6x250": 13023310,
    "sweep300x19x256": 12000446,
    "sweep23x6x250x7": 323317,
}


def delta_index(K, delta=UB_TRAINER_DELTA):
    """particle_trainer_oac.py:60-67: the first quantile i / (K - 1) >= delta."""
    for p in range(K):
        if p / (K - 1.0) >= delta:
            return p
    return None


class Case:
    def __init__(self, Do, Da, H, K=None, ub=None, delta=DELTAS[0], edge=None, n=N_ROWS,
                 tag=None):
        self.Do, self.Da, self.H, self.K, self.delta, self.edge, self.n = Do, Da, H, K, delta, edge, n
        self.ub = ub            # K heads: None (mean + beta std) or the sorted head's index
        dims = f"{Do}x{Da}x{H}" + (f"x{K}" if K else "")
        bound = "" if not K else ("-mean" if ub is None else f"-ub{ub}")
        self.name = (f"{tag}-" if tag else "") + dims + bound + (f"-{edge}" if edge else "") + \
            f"-d{delta:g}"
        # draws are shared by a shape's cases whatever the bound, delta and edge
        self.draw_key = (tag or "") + dims
        self.seed = SEED_OVERRIDES.get(self.draw_key, Do * 1000 + Da * 10 + H + (K or 0))

    @property
    def twin(self):
        return self.K is None

    @property
    def split_kernel(self):
        return not self.twin or (self.Do, self.Da, self.H) not in TWIN_KERNEL_DIMS

    @property
    def params_key(self):
        return (self.Do, self.Da, self.H, self.K, self.edge)

    def __repr__(self):
        return self.name


def _cases():
    out = []
    for delta in DELTAS:
        for d in TWIN_DIMS:
            out.append(Case(*d, delta=delta))
        for Do, Da, H, K in HEAD_DIMS:
            for ub in dict.fromkeys((None, 0, K - 1, delta_index(K))):
                out.append(Case(Do, Da, H, K, ub=ub, delta=delta))
        out.append(Case(*EDGE_TWIN, delta=delta, edge="logstd"))
        out.append(Case(*EDGE_TWIN, delta=delta, edge="zeroq"))
        out.append(Case(*EDGE_HEADS, delta=delta, edge="logstd"))
    return out


CASES = _cases()
SWEEP_CASES = [Case(Do, Da, H, K, n=max(SWEEP_NS), tag="sweep") for Do, Da, H, K in SWEEP_DIMS]
WIDE_CASE = Case(*WIDE_DIMS, n=max(WIDE_NS), tag="wide")
ALL_CASES = CASES + SWEEP_CASES + [WIDE_CASE]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


@functools.lru_cache(maxsize=None)
def params_of(key):
    """The case's parameter dicts (fp32 numpy), edge sets applied."""
    Do, Da, H, K, edge = key
    kw = dict(pi_init_w=0.2, q_init_w=0.1)
    if K:
        kw.update(q_out=K, q_last_bias=np.linspace(0.0, 50.0, K))
    p = sac_params(Do, Da, [H, H], PARAM_SEED, **kw)
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
    rows = []
    for i in range(case.n):
        if case.twin:
            r = so.oac_exploration_action(obs[i], P, Q1, Q2, BETA_UB, case.delta, zero, eps[i],
                                          dtype=dtype)
        else:
            r = so.oac_exploration_action_shared(obs[i], P, Q1, BETA_UB, case.delta, zero, eps[i],
                                                 dtype=dtype, ub_index=case.ub)
        rows.append(r)
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


def critic_forward64(case):
    """Float64 critic internals at a = tanh(mu_T) for every row: per critic
    (pre0 [n, H], pre1 [n, H], q [n, K or 1])."""
    obs, _ = inputs(case)
    p = params_of(case.params_key)
    a = np.tanh(reference(case)["mu_T"])
    x = np.concatenate([obs, a], axis=1)
    out = []
    for g in (("qf1", "qf2") if case.twin else ("qf1",)):
        q = {k: np.asarray(v, np.float64) for k, v in p[g].items()}
        pre0 = x @ q["fc0.weight"].T + q["fc0.bias"]
        pre1 = np.maximum(pre0, 0.0) @ q["fc1.weight"].T + q["fc1.bias"]
        out.append((pre0, pre1, np.maximum(pre1, 0.0) @ q["last_fc.weight"].T + q["last_fc.bias"]))
    return out


def w0_action_rms(case):
    """rms of the critics' layer-0 action columns (the scale of dQ/da)."""
    p = params_of(case.params_key)
    w = np.concatenate([np.asarray(p[g]["fc0.weight"], np.float64)[:, case.Do:].reshape(-1)
                        for g in (("qf1", "qf2") if case.twin else ("qf1",))])
    return float(np.sqrt(np.mean(w * w)))
