"""Case table of the replay side at its block edges (csrc/replay.hip,
csrc/replay_count.hip, oac_amd/replay_buffer.py) and its references.  Every
answer here is an integer or a bit pattern: the references are numpy's own
legacy RandomState stream, numpy's cumsum / searchsorted as the replay oracle
(oracle/replay_oracle.py) calls them, and ``c[idx] += 1``.

tests/test_replay_cases_cpu.py asserts the input conditions that make each
comparison well defined; tests/test_gpu_replay_edges.py runs the table on the
device.

Priority rows
  * dyadic: counts from {0, 1, 3, 7} (weights 1, 1/2, 1/4, 1/8), arranged so
    that the total weight is a power of two.  Every partial sum is then a
    multiple of 1/8 below 2^23: exact in float64 in any association, the
    oracle's normalisation is an exact power-of-two scaling, and so is the
    device's u * total.  The device must agree for every u, ties included.
  * general: randint(0, 40) counts.  The device scan associates differently
    from numpy's sequential cumsum, so a draw must keep a margin from every
    cdf step (MARGIN x the float64 cdf's own distance from a long double one).
"""
from collections import namedtuple

import numpy as np

from oracle.replay_oracle import CountReplayOracle

SCAN_BLOCK = 4096                 # csrc/replay_count.hip kScanBlock
MAX_SIZE = SCAN_BLOCK * 1024      # the size oac_replay_priority_sample admits
MARGIN = 1000.0                   # general rows: distance to a cdf step / cdf rounding
DYADIC_COUNTS = (0, 1, 3, 7)
TIE_ROWS = (0, 4094, 4095, 4096)  # and size - 2
N_RANDOM_U = 300

Dyadic = namedtuple("Dyadic", "name size capacity seed")
General = namedtuple("General", "name size B seed")

DYADIC = [Dyadic(f"dyadic-{n}", n, n, 100 + i) for i, n in enumerate(
    [1, 2, 4095, 4096, 4097, 8192, 8193, 3 * SCAN_BLOCK + 1, MAX_SIZE])]
DYADIC.append(Dyadic("dyadic-4097-of-10000", 4097, 10000, 120))
# seeds chosen on the CPU (test_replay_cases_cpu.py) so that every draw keeps the margin
GENERAL = [General("general-4095", 4095, 1000, 1), General("general-4097", 4097, 1000, 1),
           General("general-8193", 8193, 2048, 1), General("general-200003", 200003, 4096, 1)]
DYADIC_BY_NAME = {c.name: c for c in DYADIC}
GENERAL_BY_NAME = {c.name: c for c in GENERAL}


class _FixedUniforms:
    """Stands in for numpy's global stream in CountReplayOracle.indices."""

    def __init__(self, u):
        self.u = u

    def random_sample(self, B):
        assert B == len(self.u)
        return self.u


def oracle_indices(counts, u):
    """CountReplayOracle's priority draw for these counts and uniforms."""
    o = CountReplayOracle(len(counts), 1, 1, priority_sample=True)
    o.counts[:, 0] = counts
    o.size = len(counts)
    idx, u2 = o.indices(len(u), rng=_FixedUniforms(u))
    assert u2 is u
    return idx.astype(np.int64)


def oracle_cdf(counts):
    """The cdf CountReplayOracle.indices searches, same operations."""
    probs = 1 / (np.asarray(counts, np.float64).reshape(-1, 1) + 1)
    probs /= probs.sum()
    cdf = probs[:, 0].cumsum()
    cdf /= cdf[-1]
    return cdf


def dyadic_class_sizes(size):
    """(n0, n1, n3, n7) rows of count 0, 1, 3, 7 with n0 + n1 + n3 + n7 = size
    and 8 n0 + 4 n1 + 2 n3 + n7 = 8 * 2^k, as many classes present as the size
    allows.  Two rows are set by hand: 4097 = 4095 rows of count 0 and two of
    count 1 (total 4096), 4,194,304 = 2^20 of count 0, 2^20 of count 1 and
    2^21 of count 3 (total 2^21)."""
    if size == 4097:
        return (4095, 2, 0, 0)
    if size == MAX_SIZE:
        return (1 << 20, 1 << 20, 1 << 21, 0)
    best = None
    T = 1
    while T <= size:
        for n7 in range(0, min(size, 64) + 1, 2):
            for n3 in range(0, min(size - n7, 64) + 1):
                S, R = size - n3 - n7, 8 * T - 2 * n3 - n7
                if R < 0 or (R - 4 * S) % 4:
                    continue
                n0 = (R - 4 * S) // 4
                n1 = S - n0
                if n0 < 0 or n1 < 0:
                    continue
                cand = (sum(1 for n in (n0, n1, n3, n7) if n), T, n3 + n7, (n0, n1, n3, n7))
                if best is None or cand > best:
                    best = cand
        T *= 2
    assert best is not None, size
    return best[3]


def dyadic_counts(case):
    """int32 counts [capacity]: the first ``size`` rows are the permuted
    dyadic row; rows past the size (never valid) hold count 0, weight 1, so a
    scan that read them would move every index."""
    rs = np.random.RandomState(case.seed)
    c = np.repeat(np.array(DYADIC_COUNTS, np.int32), dyadic_class_sizes(case.size))
    c = c[rs.permutation(case.size)]
    out = np.zeros(case.capacity, np.int32)
    out[:case.size] = c
    return out


def tie_rows(size):
    return sorted({j for j in TIE_ROWS + (size - 2,) if 0 <= j <= size - 2})


def dyadic_uniforms(case):
    """(u, tie) -- u: 0, the largest double below 1, cdf[j] and the next double
    below it for every tie row j, then N_RANDOM_U random_sample draws;
    tie: [(j, position of cdf[j] in u, position of its predecessor)]."""
    cdf = oracle_cdf(dyadic_counts(case)[:case.size])
    u = [0.0, 1.0 - 2.0 ** -53]
    tie = []
    for j in tie_rows(case.size):
        tie.append((j, len(u), len(u) + 1))
        u += [cdf[j], np.nextafter(cdf[j], 0.0)]
    rs = np.random.RandomState(case.seed + 1000)
    return np.concatenate([np.array(u, np.float64), rs.random_sample(N_RANDOM_U)]), tie


_DYADIC_REF = {}


def dyadic_reference(case):
    """(counts [capacity], u, expected indices, tie), computed once per row."""
    if case.name not in _DYADIC_REF:
        counts = dyadic_counts(case)
        u, tie = dyadic_uniforms(case)
        idx = oracle_indices(counts[:case.size], u)
        for a in (counts, u, idx):
            a.setflags(write=False)
        _DYADIC_REF[case.name] = (counts, u, idx, tie)
    return _DYADIC_REF[case.name]


def general_counts(case):
    return np.random.RandomState(case.seed).randint(0, 40, case.size).astype(np.int32)


def general_uniforms(case):
    """What np.random.seed(case.seed + 1); random_sample(B) draws: the GPU
    test seeds the global stream so and calls _priority_indices."""
    return np.random.RandomState(case.seed + 1).random_sample(case.B)


_GENERAL_REF = {}


def general_reference(case):
    if case.name not in _GENERAL_REF:
        counts, u = general_counts(case), general_uniforms(case)
        idx = oracle_indices(counts, u)
        for a in (counts, u, idx):
            a.setflags(write=False)
        _GENERAL_REF[case.name] = (counts, u, idx)
    return _GENERAL_REF[case.name]


def general_margin_ratio(case):
    """min over the draws of (distance to the nearest cdf step) / (largest
    difference between the float64 cdf and the same cdf in long double)."""
    counts, u = general_counts(case), general_uniforms(case)
    cdf = oracle_cdf(counts)
    p = 1 / (counts.astype(np.longdouble) + 1)
    p /= p.sum()
    cl = np.cumsum(p)
    cl /= cl[-1]
    noise = float(np.max(np.abs(cl - cdf.astype(np.longdouble))))
    k = np.searchsorted(cdf, u, side="right")
    below = np.where(k > 0, u - cdf[np.maximum(k - 1, 0)], np.inf)
    above = cdf[np.minimum(k, len(cdf) - 1)] - u
    return float(min(below.min(), above.min())) / noise, noise


# ----------------------------------------------------------------- counts
COUNT_ROWS = 50
COUNT_BATCHES = (1, 255, 256, 257, 1025, 4096)
RING_COUNT_ROWS = 300


def bump(counts, idx):
    """numpy's buffered fancy-index update: a repeated index counts once.
    Returns the batch counts before the update."""
    before = counts[idx].copy()
    counts[idx] += 1
    return before


# ---------------------------------------------------------------- MT19937
MT_COUNTS = (0, 1, 623, 624, 625, 0, 1247, 1, 1249, 624)   # the ends of a 624-word block
MT_SEQUENCE_SIZES = (1000, (1 << 20) + 1)
MT_SINGLE_SIZES = (1 << 32, (1 << 31) + 1, 1 << 16, (1 << 16) - 1, (1 << 16) + 1)
MT_SINGLE_COUNT = 1500


def randint_calls(seed, size, counts):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, size, n) for n in counts]


# ------------------------------------------------------- insert and gather
INSERT_SHAPES = ((4, 2), (3, 4), (376, 17))   # row strides 12, 12 (no pad columns), 772
INSERT_CAPACITY = 5
INSERT_LENGTHS = (3, 4, 5, 11)
GATHER_SHAPES = ((1, 1), (376, 17))           # 2 and 193 float4 per row
GATHER_BATCHES = (1, 15, 16, 17, 250)         # kGatherRows = 16
GATHER_ROWS = 97


def gather_indices(B, seed=0):
    """Row 0, the last row and duplicates, in a random order."""
    rs = np.random.RandomState(seed + B)
    idx = rs.randint(0, GATHER_ROWS, B)
    if B >= 4:
        idx[:4] = [GATHER_ROWS - 1, 0, 5, 5]
        rs.shuffle(idx)
    elif B == 1:
        idx[0] = GATHER_ROWS - 1
    return idx.astype(np.int32)


# ------------------------------------------------------------ index stream
STREAM_ROWS, STREAM_B, STREAM_CHUNK = 1000, 37, 4
STREAM_BLOCKS = (1, 1, 2, 4, 4, 2, 2, 1, 1, 1, 1, 4)   # 24 steps = 6 chunks, every block
#                                                        inside a multiple of its length
assert sum(STREAM_BLOCKS) == 6 * STREAM_CHUNK


def stream_draws(seed, steps, size=STREAM_ROWS, B=STREAM_B):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, size, B) for _ in range(steps)]
