"""CPU restatement of ReplayBufferNoResampling (the reference's
replay_buffer_no_resampling.py) for the tests -- arrays only, no ``list.remove``
-- the Floyd position draw of oac_replay_nr_sample_positions on
oracle/philox_oracle.py with Python integers, the fixtures' paths, and the case
tables of tests/test_gpu_noresample.py (checked on the CPU by
tests/test_noresample_cpu.py)."""
import numpy as np

from oracle.philox_oracle import philox4x32_10

GOLDENS = ("noresample_schedule", "noresample_ragged", "noresample_n257", "noresample_n4097")
FIELDS = ("observations", "actions", "rewards", "next_observations", "terminals")
NR_STREAM = 4          # the draw's Philox stream id (csrc/replay_noresample.hip kNrStream)
MAX_B = 4096


def make_path(rs, T, obs_dim, act_dim):
    """One rollout path of T rows from the RandomState ``rs``: float64 values
    that float32 cannot represent, drawn from a pool of 64 (the fixtures' final
    arrays then compress), terminals bool [T, 1]."""
    pool = rs.standard_normal(64) * np.pi
    assert not np.array_equal(pool, pool.astype(np.float32).astype(np.float64))
    f = lambda *shape: pool[rs.randint(0, 64, shape)]   # noqa: E731
    return dict(observations=f(T, obs_dim), actions=f(T, act_dim), rewards=f(T, 1),
                next_observations=f(T, obs_dim), terminals=(rs.uniform(0, 1, (T, 1)) < 0.2),
                agent_infos=[{}] * T, env_infos=[{}] * T)


class NoResampleOracle:
    """The reference's state machine on arrays.  ``valid`` is the ordered live
    list, ``queue`` the uint64 ring of freed slots; the three ring counters move
    with the reference's own arithmetic (N freed slots alias to 'empty')."""

    def __init__(self, N, obs_dim=0, act_dim=0):
        self.N = int(N)
        self.valid = np.zeros(0, np.int64)
        self.queue = np.zeros(self.N, np.uint64)
        self.top = self.bottom = self.top_idx = self.size = 0
        self.fields = dict(observations=np.zeros((N, obs_dim)), actions=np.zeros((N, act_dim)),
                           rewards=np.zeros((N, 1)), next_observations=np.zeros((N, obs_dim)),
                           terminals=np.zeros((N, 1), np.uint8))

    def slots_for(self, m):
        """The slots the next m add_sample calls write, in order (:98-122)."""
        N = self.N
        q = (self.top_idx - self.bottom) % N
        s = np.arange(m)
        from_queue = self.queue[(self.bottom + s) % N]   # read for every s, used for s < q
        return np.where(s < q, from_queue.astype(np.int64), (self.top + s - q) % N)

    def add(self, m, path=None):
        N = self.N
        assert len(self.valid) + m <= N, "the schedule exceeds the capacity"
        slots = self.slots_for(m)
        k = min(m, (self.top_idx - self.bottom) % N)
        self.bottom = (self.bottom + k) % N
        self.top = (self.top + m - k) % N
        self.size = min(self.size + m, N)
        self.valid = np.concatenate([self.valid, slots])
        if path is not None:
            for key in FIELDS:
                self.fields[key][slots] = np.asarray(path[key]).reshape(m, -1)
        return slots

    def take(self, positions):
        """random_batch's bookkeeping for the given list positions (:124-141)."""
        pos = np.asarray(positions, np.int64)
        B, N = len(pos), self.N
        idx = self.valid[pos]
        self.queue[(self.top_idx + np.arange(B)) % N] = idx.astype(np.uint64)
        self.top_idx = (self.top_idx + B) % N
        self.valid = np.delete(self.valid, pos)
        self.size -= B
        return idx

    def counters(self):
        return [self.top, self.bottom, self.top_idx, self.size]


def floyd_positions(n, B, seed, draw):
    """B distinct positions of [0, n): for t = 0 .. B-1, j = n - B + t, Philox
    counter {t, 4, draw lo, draw hi} under key = seed, w = (word0 << 32) | word1,
    r = (w * (j + 1)) >> 64, pick r unless already picked, then j."""
    n, B, seed, draw = int(n), int(B), int(seed), int(draw)
    assert 1 <= B <= n
    t = np.arange(B, dtype=np.uint64)
    z = np.zeros(B, np.uint64)
    c = philox4x32_10([t, z + np.uint64(NR_STREAM), z + np.uint64(draw & 0xFFFFFFFF),
                       z + np.uint64((draw >> 32) & 0xFFFFFFFF)],
                      [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    picks, seen = [], set()
    for k in range(B):
        w = (int(c[0][k]) << 32) | int(c[1][k])
        j = n - B + k
        r = (w * (j + 1)) >> 64
        p = j if r in seen else r
        seen.add(p)
        picks.append(p)
    return np.asarray(picks, np.int64)


# ------------------------------------------------------------- case tables
CHUNK = 256   # list elements per compaction workgroup (oac_replay_nr_chunk)
TAKE_LENGTHS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 3 * CHUNK + 1)
TAKE_BS = (1, 2, 63, 64, 65, 1024, 4096)


def take_cases():
    """(name, list length, positions) of the compaction-edge sweep: the named
    removal sets, then every B of TAKE_BS that fits, as a shuffled draw and as
    a descending run."""
    cases = []
    for n in TAKE_LENGTHS:
        sets = {"first": [0], "last": [n - 1], "all": list(range(n))}
        if n >= 2:
            sets["both"] = [0, n - 1]
            sets["every_other"] = list(range(0, n, 2))
        edges = [e for e in range(CHUNK, n, CHUNK)]
        for e in edges:   # a run of 5 that straddles the block edge e
            sets[f"straddle{e}"] = [p for p in range(e - 2, e + 3) if p < n]
        for name, pos in sets.items():
            if len(pos) > MAX_B:
                continue
            cases.append((f"n{n}-{name}-desc", n, np.asarray(pos[::-1], np.int64)))
            rs = np.random.RandomState(n * 31 + len(pos))
            cases.append((f"n{n}-{name}-shuf", n, rs.permutation(np.asarray(pos, np.int64))))
        for B in TAKE_BS:
            if B > n:
                continue
            rs = np.random.RandomState(n * 131 + B)
            pos = rs.permutation(n)[:B].astype(np.int64)
            cases.append((f"n{n}-B{B}-shuf", n, pos))
            cases.append((f"n{n}-B{B}-desc", n, np.sort(pos)[::-1].copy()))
    return cases


DRAW_CASES = ((1, 1), (2, 2), (5, 5), (64, 64), (65, 64), (1000, 1), (4097, 1024), (4096, 4096),
              (1_000_000, 256))
DRAW_COUNTERS = (0, 1, 2 ** 32)
