"""The one-hidden-layer gradient steps' width and action sweep (test
infrastructure, no GPU): which (Do, Da, H, B, K) tests/test_gpu_shallow_wide.py
runs through the three depth-1 step families, the state and inputs of each row,
its CPU oracles, the input conditions under which the comparison leaves no
element out (tests/test_shallow_wide_cases_cpu.py asserts them for every row),
and the kernel branches each row reaches, recomputed from the constants of
csrc/rows.hip and the plans.

Families: 'sac' (ShallowSACTrainer, auto_alpha), 'goac' / 'ptrain' (the shared
depth-1 GaussianTrainer with K = 2 / ParticleTrainer, counts=True), 'us_goac' /
'us_ptrain' (share_layers=False; their kernels see the stacked width K H).

State: fixtures_lib parameters at the row's seed with pi_init_w = 0.05 (mean
head small enough for |tanh| < 0.999) and q_init_w = 0.1, a mid-training
optimiser state (fixtures_lib.mid_state, t = 7, seed + 1); the batch is B rows
of fixtures_lib.synthetic_transitions(seed + 2) with 0/1 counts; SAC's eps are
0.5 x standard normal draws (the batch path takes any eps).
"""
import contextlib
import functools

import numpy as np
import torch

import sac_shallow_lib as ssl
import shallow_lib as sl
import unshared_oracle as uo
from fixtures_lib import synthetic_transitions
from oracle import sac_oracle as so

T_MID = 7
DELTA = 0.95
MARGIN = 8.0           # the mask / rank condition: 8 x the fp32-to-float64 discrepancy
MAX_SEEDS = 20
TANH_MAX = 0.999

# name: (Do, Da, H, B) -- the issue's table; what each reaches is recomputed by
# reaches() below and asserted in tests/test_shallow_wide_cases_cpu.py
STEP_CASES = {
    "w64": (3, 3, 64, 17),
    "w68": (4, 4, 68, 16),
    "da9": (11, 9, 128, 33),
    "da16": (5, 16, 32, 48),
    "w252": (23, 6, 252, 37),
    "da32": (17, 32, 260, 19),
    "humanoid": (376, 17, 256, 37),
    "w512": (376, 17, 512, 19),
    "slabs": (23, 6, 68, 600),
}
PTRAIN_K = dict(w64=10, w68=10, da9=10, da16=10, w252=10, humanoid=16, da32=3, w512=5, slabs=5)
# The large-batch kernel set (B >= 1024), once per family.  Narrower than w252
# at B = 1100: there the input condition cannot be met -- 250 k to 3 M hidden
# pre-activations per evaluation, and over 20 seeds the best margin of any of
# the four kinds was 0.28 of the required 1 (0.7 at (23, 6, 132, 1030)).  These
# keep a ragged last row block, a width that is a multiple of 4 only and two
# 128-column head chunks (132; 2 x 68 stacked), and meet it.
LARGE_SHARED = ("b1030", (5, 6, 132, 1030))
LARGE_SEPARATE = ("b1030", (5, 6, 68, 1030))
# separate critics: (family, name, (Do, Da, H, B), K) -- the stacked width is K H
UNSHARED_CASES = [
    ("us_goac", "s512", (376, 17, 256, 37), 2),
    ("us_ptrain", "s600", (23, 6, 60, 37), 10),
    ("us_ptrain", "s320", (5, 16, 20, 33), 16),
    ("us_ptrain", "s264", (17, 32, 88, 19), 3),
]

# row id -> a seed (of the MAX_SEEDS from the row's base seed) that meets every
# input condition: find_seed(row), run on the CPU when a row is added
SEEDS = {
    "sac-w64": 9601, "sac-w68": 301, "sac-da9": 2801, "sac-da16": 7401, "sac-w252": 4601,
    "sac-da32": 7202, "sac-humanoid": 4508, "sac-w512": 4517, "sac-slabs": 1620,
    "goac-w64": 101, "goac-w68": 501, "goac-da9": 3001, "goac-da16": 7601, "goac-w252": 4805,
    "goac-da32": 7401, "goac-humanoid": 4702, "goac-w512": 4718, "goac-slabs": 1815,
    "goac-b1030": 7019,
    "ptrain-w64": 5101, "ptrain-w68": 5509, "ptrain-da9": 8002, "ptrain-da16": 2901,
    "ptrain-w252": 102, "ptrain-da32": 2701, "ptrain-humanoid": 10, "ptrain-w512": 2,
    "ptrain-slabs": 6814, "ptrain-b1030": 2305,
    "us_goac-s512": 7905, "us_ptrain-s600": 3001, "us_ptrain-s320": 2903, "us_ptrain-s264": 3601,
    "us_goac-b1030": 918,
}


class Row:
    def __init__(self, family, name, dims, K):
        self.family, self.name, self.K = family, name, K
        self.Do, self.Da, self.H, self.B = dims
        self.id = f"{family}-{name}"

    @property
    def base_seed(self):
        return 100 * (sum(map(ord, self.id)) % 97) + 1

    @property
    def seed(self):
        return SEEDS[self.id]

    @property
    def unshared(self):
        return self.family.startswith("us_")

    @property
    def kind(self):
        return None if self.family == "sac" else self.family.replace("us_", "")

    @property
    def width(self):
        """The hidden width the row kernels see: H, or K H stacked critics."""
        return self.K * self.H if self.unshared else self.H

    def __repr__(self):
        return self.id


def _rows():
    out = [Row("sac", n, d, None) for n, d in STEP_CASES.items()]
    for n, d in list(STEP_CASES.items()) + [LARGE_SHARED]:
        out.append(Row("goac", n, d, 2))
        out.append(Row("ptrain", n, d, PTRAIN_K.get(n, 10)))
    out += [Row(f, n, d, K) for f, n, d, K in UNSHARED_CASES]
    out.append(Row("us_goac", LARGE_SEPARATE[0], LARGE_SEPARATE[1], 2))
    return out


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
FAMILY_GROUPS = {"sac": ("sac",), "shared": ("goac", "ptrain"), "separate": ("us_goac", "us_ptrain")}


def rows_of(group):
    return [r for r in ROWS if r.family in FAMILY_GROUPS[group]]


def delta_index(K, delta=DELTA):
    """particle_trainer.py:61-69: the quantile i / (K - 1) at delta, or the one below it."""
    for p in range(K):
        q = p * 1.0 / (K - 1)
        if q == delta:
            return p
        if q > delta:
            return p - 1
    return None


# --------------------------------------------------------- state and inputs
def meta_of(row, seed=None):
    seed = row.seed if seed is None else seed
    m = dict(obs_dim=row.Do, act_dim=row.Da, hidden=[row.H], seed=seed, pi_init_w=0.05, q_init_w=0.1,
             discount=0.99, tau=5e-3)
    if row.family == "sac":
        m.update(reward_scale=1.0, lr=1e-3, auto_alpha=True, log_alpha0=0.0, target_update_period=1,
                 mid_state=dict(t=T_MID, seed=seed + 1))
        return m
    m.update(kind=row.kind, K=row.K, q_min=0.0, q_max=50.0, delta=DELTA, lr=3e-4, std_lr=1e-4,
             counts=True, n_replay=400)
    if row.kind == "ptrain":
        m["delta_index"] = delta_index(row.K)
    return m


def params_of(row, seed=None):
    meta = meta_of(row, seed)
    if row.family == "sac":
        return ssl.params_of(meta)
    return uo.params_of(meta) if row.unshared else sl.params_of(meta)


def _adam_groups(row, params):
    """{group name: parameter dict} of the det trainers' Adam groups."""
    g = dict(policy=params["policy"], target_policy=params["target_policy"])
    if row.unshared:
        g.update({f"qf{k}": p for k, p in enumerate(params["qfs"])})
    else:
        g["qf"] = params["qf1"]
    return g


def mid_state_of(row, seed=None):
    """The det families' mid-training state (SAC's is in its meta)."""
    seed = row.seed if seed is None else seed
    return sl.det_mid_state(_adam_groups(row, params_of(row, seed)), T_MID, seed + 1)


def batch_of(row, seed=None):
    """(batch, eps1, eps2): eps None for the deterministic-policy families."""
    seed = row.seed if seed is None else seed
    B, Do, Da = row.B, row.Do, row.Da
    data = synthetic_transitions(max(4 * B, 64), Do, Da, seed=seed + 2)
    idx = np.random.RandomState(seed + 3).randint(0, len(data["rewards"]), B)
    b = {k: v[idx] for k, v in data.items()}
    rs = np.random.RandomState(seed + 4)
    if row.family == "sac":
        e = [(0.5 * rs.standard_normal((B, Da))).astype(np.float32) for _ in range(2)]
        return b, e[0], e[1]
    b["counts"] = rs.randint(0, 2, (B, 1)).astype(np.float64)
    return b, None, None


def oracle_of(row, dtype, seed=None):
    """The row's CPU oracle at its mid-training state."""
    meta = meta_of(row, seed)
    if row.family == "sac":
        return ssl.make_oracle(meta, dtype)
    params = params_of(row, seed)
    ms = mid_state_of(row, seed)
    if row.unshared:
        orc = uo.make_oracle(meta, dtype, params=params)
        opts = dict(policy=orc.opt_p, target_policy=orc.opt_tp)
        opts.update({f"qf{k}": o for k, o in enumerate(orc.opts)})
    else:
        orc = sl.make_oracle(meta, dtype, params=params)
        opts = dict(policy=orc.opt_p, target_policy=orc.opt_tp, qf=orc.opt_q)
    sl.load_oracle_mid_state(orc, opts, ms)
    return orc


def step(orc, row, seed=None):
    b, e1, e2 = batch_of(row, seed)
    return orc.step(b, e1, e2) if row.family == "sac" else orc.step(b)


def trainer_of(row):
    """The oac_amd trainer of the row at its mid-training state (GPU)."""
    meta = meta_of(row)
    if row.family == "sac":
        return ssl.trainer_for(meta)
    params = params_of(row)
    tr = uo.trainer_for(meta, params=params) if row.unshared else sl.trainer_for(meta, params=params)
    mods = dict(policy=tr.policy, target_policy=tr.target_policy)
    if row.unshared:
        mods.update({f"qf{k}": q for k, q in enumerate(tr.qfs)})
    else:
        mods["qf"] = tr.qfs[0]
    sl.load_mid_state(tr, mods, mid_state_of(row))
    return tr


# --------------------------------------------------------- input conditions
@contextlib.contextmanager
def recorded(log):
    """While active, every hidden-layer evaluation an oracle step makes
    (oracle.sac_oracle.mlp_trunk: the policies and critics of every family go
    through it) appends its layer-0 pre-activation to log['pre'], every policy
    forward its action to log['a'], every critic forward its output to log['q']."""
    trunk, pol, qf = so.mlp_trunk, so.policy_forward, so.q_forward

    def mlp_trunk(x, p):
        assert so.n_hidden(p) == 1
        log.setdefault("pre", []).append(so.linear(x, p["fc0.weight"], p["fc0.bias"]).double())
        return trunk(x, p)

    def policy_forward(*a, **kw):
        out = pol(*a, **kw)
        log.setdefault("a", []).append(out["a"].double())
        return out

    def q_forward(*a, **kw):
        out = qf(*a, **kw)
        log.setdefault("q", []).append(out["q"].double())
        return out

    so.mlp_trunk, so.policy_forward, so.q_forward = mlp_trunk, policy_forward, q_forward
    try:
        yield log
    finally:
        so.mlp_trunk, so.policy_forward, so.q_forward = trunk, pol, qf


def n_evaluations(row):
    """Hidden-layer evaluations per step: the policy on obs and next_obs (and
    the target policy on obs), the critics on (obs, a), (obs, a~) (and on the
    target policy's action), the targets on (next_obs, a')."""
    if row.family == "sac":
        return 2 + 3 * 2                  # the policy twice; both critics on (obs, a), (obs, a~); both targets
    if row.family == "us_goac":
        return 3 + 3 * 2 + 1              # (the target policy's action goes through q alone)
    n = row.K if row.unshared else 1
    return 3 + 4 * n


def conditions(row, seed=None):
    """The row's input conditions on the two CPU oracles at ``seed``:
    dict(mask=smallest |pre64| / b over every hidden-layer evaluation with b =
    MARGIN max|pre32 - pre64| of that evaluation, rank=the same for the
    particle rows' smallest rank gap (inf otherwise), tanh=largest |a| of any
    policy forward in float64).  mask > 1, rank > 1 and tanh < TANH_MAX hold
    for the seed the table stores."""
    logs = {}
    for dt in (torch.float32, torch.float64):
        with recorded({}) as log:
            step(oracle_of(row, dt, seed), row, seed)
        logs[dt] = log
    l32, l64 = logs[torch.float32], logs[torch.float64]
    assert len(l32["pre"]) == len(l64["pre"]) == n_evaluations(row)
    mask = np.inf
    for a, b in zip(l32["pre"], l64["pre"]):
        bound = MARGIN * float((a - b).abs().max())
        mask = min(mask, float(b.abs().min()) / max(bound, 1e-300))
    rank = np.inf
    if row.kind == "ptrain":
        q32, q64 = l32["q"], l64["q"]
        if row.unshared:     # K one-output critics per evaluation, in order (unshared_oracle._stack)
            K = row.K
            q32 = [torch.cat(q32[i:i + K], 1) for i in range(0, len(q32), K)]
            q64 = [torch.cat(q64[i:i + K], 1) for i in range(0, len(q64), K)]
        for a, b in zip(q32, q64):            # [B, K] each
            s = torch.sort(b, dim=1)[0]
            spread = float((s[:, -1] - s[:, 0]).min())
            disc = MARGIN * float((a - b).abs().max()) / spread
            rank = min(rank, uo.min_rank_gap(b.t()) / max(disc, 1e-300))
    tanh = max(float(a.abs().max()) for a in l64["a"])
    return dict(mask=mask, rank=rank, tanh=tanh)


def conditions_hold(c):
    return c["mask"] > 1.0 and c["rank"] > 1.0 and c["tanh"] < TANH_MAX


def find_seed(row):
    """Of the MAX_SEEDS seeds from the row's base seed (a bounded search, as the
    golden generators' gen_checked) the one that meets the conditions with the
    largest mask margin, or None."""
    best = None
    for s in range(row.base_seed, row.base_seed + MAX_SEEDS):
        c = conditions(row, s)
        if conditions_hold(c) and (best is None or c["mask"] > best[1]):
            best = (s, c["mask"])
    return None if best is None else best[0]


@functools.lru_cache(maxsize=None)
def stored_conditions(row_id):
    return conditions(BY_ID[row_id])


# --------------------------------------------------------- branch coverage
def reaches(row):
    """What the row's shape selects in the depth-1 kernels, recomputed from
    (Da, H, B, K) -- these restate constants of the sources cited."""
    Da, B, W = row.Da, row.B, row.width
    # rows.hip:1019-1023 / 1306-1310: Dp = the power of two >= min(Da, 16); lane
    # jl takes dims jl (acc0) and jl + 16 (acc1, live for jl + 16 < Da)
    Dp = 1
    while Dp < Da and Dp < 16:
        Dp <<= 1
    # rows.hip:975 kDshChunk = 256, :1025-1026 / :1318-1319 the chunk loop over the
    # width the kernel sees (H; K H for the block-diagonal last layer, :1030-1031)
    n_chunks = -(-W // 256)
    # rows.hip:316 the one-batch form of row_heads (H % 16 == 0 and H <= 256, H / 16
    # k-chunks), else the generic loop (:337-366) over ceil(H / 16) chunks
    fast = W % 16 == 0 and W <= 256
    # sac_shallow_plan.hip:128, det_plan.hip:153 / :486: head column chunks of the
    # (stacked) hidden width, 64 columns below B = 1024, 128 from there
    per = 128 if B >= 1024 else 64
    col_chunks = max(1, -(-W // per))
    nbw = -(-W // 64)       # rows.hip:1076, :1082 seg_last_update_kernel's column workgroups
    return dict(
        Dp=Dp, lanes_live=min(Da, 16), acc1_lanes=max(0, Da - 16),
        n_chunks=n_chunks, last_chunk=W - 256 * (n_chunks - 1),
        heads_path="fast" if fast else "generic", heads_chunks=-(-W // 16),
        col_chunks=col_chunks, cols_per_chunk=-(-W // col_chunks),
        # plan_common.h:66-78 choose_split: slabs from B = 512 (these rows' tile counts
        # are far below 512), sac_plan.h:137-139 can_fuse_adam: no slabs, small-batch set
        fused=B < 512, large_batch=B >= 1024,              # plan_api.hip:330
        row_blocks=-(-B // 16), ragged_rows=B % 16 != 0,   # rows.hip:285 kRowBlock = 16
        seg_workgroups=nbw, seg_last_cols=W - 64 * (nbw - 1),
        partial_gemm_tile=row.H % 32 != 0, mult4_only=row.H % 8 == 4)
