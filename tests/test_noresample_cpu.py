"""ReplayBufferNoResampling on the CPU: the array restatement
(tests/noresample_oracle.py) against every state the reference recorded
(tests/golden/noresample_*.npz), the preconditions of the GPU case tables, the
Floyd draw's restatement, and the new entry points' refusals (host-only: they
fail before any launch, with null buffers)."""
import ctypes

import numpy as np
import pytest

import parity
from noresample_oracle import (DRAW_CASES, GOLDENS, MAX_B, TAKE_BS, TAKE_LENGTHS, CHUNK,
                               NoResampleOracle, floyd_positions, make_path, take_cases)


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_equals_every_recorded_state(name):
    meta, g = parity.load(name)
    N = meta["N"]
    orc = NoResampleOracle(N, meta["obs_dim"], meta["act_dim"])
    rs = np.random.RandomState(meta["data_seed"])
    np.random.seed(meta["np_seed"])
    crossed = set()
    for k, (what, n) in enumerate(meta["ops"]):
        live = len(orc.valid)
        if what == "add":
            assert live + n <= N, f"op {k}: the schedule exceeds the capacity"
            orc.add(n, make_path(rs, n, meta["obs_dim"], meta["act_dim"]))
        else:
            assert 1 <= n <= live
            # the reference's draw IS a draw of positions on the same stream
            pos = np.random.choice(live, size=n, replace=False)
            idx = orc.take(pos)
            np.testing.assert_array_equal(idx, g[f"op{k}/idx"], err_msg=f"op {k}")
        crossed.add(len(orc.valid))
        np.testing.assert_array_equal(orc.valid, g[f"op{k}/valid"], err_msg=f"op {k} list")
        np.testing.assert_array_equal(orc.queue, g[f"op{k}/queue"].astype(np.uint64),
                                      err_msg=f"op {k} ring")
        assert orc.counters() == g[f"op{k}/counters"].tolist(), f"op {k}"
        assert len(set(orc.valid.tolist())) == len(orc.valid)
    for key, gk in (("observations", "observations"), ("actions", "actions"),
                    ("rewards", "rewards"), ("terminals", "terminals"),
                    ("next_observations", "next_obs")):
        np.testing.assert_array_equal(orc.fields[key], g[f"final/{gk}"], err_msg=key)
    assert np.random.randint(2 ** 31) == int(g["final/randint"])
    # each schedule reaches what it is for
    if name == "noresample_ragged":
        assert 0 in crossed and N in crossed, "a full drain and a refill"
    if name in ("noresample_n257", "noresample_n4097"):
        assert N in crossed and any(c < N - 1 for c in crossed), "both sides of N - 1"
    if name == "noresample_schedule":
        assert max(crossed) == N and N == 5 * 20 * 4


def test_choice_of_a_list_is_a_choice_of_positions():
    """np.random.choice(lst, B, replace=False) == lst[np.random.choice(len, B,
    replace=False)] == lst[permutation(len)[:B]], with the stream left equal."""
    for n, B in ((50, 7), (4097, 256)):
        lst = np.random.RandomState(n).permutation(3 * n)[:n].tolist()
        got, after = [], []
        for draw in (lambda: np.random.choice(lst, size=B, replace=False),
                     lambda: np.asarray(lst)[np.random.choice(len(lst), size=B, replace=False)],
                     lambda: np.asarray(lst)[np.random.permutation(len(lst))[:B]]):
            np.random.seed(9)
            got.append(np.asarray(draw()))
            after.append(np.random.randint(2 ** 31))
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
        assert after[0] == after[1] == after[2]


def test_case_tables_hold_their_preconditions():
    assert TAKE_LENGTHS[-1] == 3 * CHUNK + 1
    cases = take_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    seen_b, seen_n = set(), set()
    for name, n, pos in cases:
        assert 1 <= len(pos) <= min(n, MAX_B), name
        assert pos.min() >= 0 and pos.max() < n and len(np.unique(pos)) == len(pos), name
        seen_b.add(len(pos))
        seen_n.add(n)
    assert set(TAKE_BS) <= seen_b and set(TAKE_LENGTHS) == seen_n
    assert any(len(pos) == n for _, n, pos in cases), "a take that empties the list"
    assert any("straddle" in nm for nm in names)
    for n, B in DRAW_CASES:
        assert 1 <= B <= min(n, MAX_B)


@pytest.mark.parametrize("n,B", [(1, 1), (2, 2), (5, 5), (64, 64), (65, 64), (1000, 1),
                                 (4097, 1024), (1_000_000, 256)])
def test_floyd_restatement_gives_distinct_picks_in_range(n, B):
    for d in (0, 1, 2 ** 32):
        p = floyd_positions(n, B, seed=77, draw=d)
        assert len(p) == B and len(set(p.tolist())) == B and p.min() >= 0 and p.max() < n
        if B == n:
            assert sorted(p.tolist()) == list(range(n))


def test_floyd_restatement_spreads_single_elements_evenly():
    """n = 10, B = 3 over 20,000 draw counters: every element is picked with
    frequency 0.3, each within 5 standard deviations (a condition, not a
    measurement: sd = sqrt(0.3 * 0.7 / 20000))."""
    T = 20000
    hits = np.zeros(10)
    for d in range(T):
        hits[floyd_positions(10, 3, seed=12345, draw=d)] += 1
    sd = np.sqrt(0.3 * 0.7 / T)
    assert np.all(np.abs(hits / T - 0.3) < 5 * sd), hits / T


def test_parallel_collision_rule_equals_the_sequential_draw():
    """The kernel resolves the draw without a sequential pass: step t collides
    iff an earlier step drew the same r, or r == j_s of an earlier step s that
    collided itself.  Restated here on the restatement's own r values."""
    from oracle.philox_oracle import philox4x32_10
    for n, B, d in ((5, 5, 0), (64, 64, 3), (70, 64, 1), (300, 256, 2), (2048, 2048, 0)):
        t = np.arange(B, dtype=np.uint64)
        z = np.zeros(B, np.uint64)
        c = philox4x32_10([t, z + np.uint64(4), z + np.uint64(d), z], [77, 0])
        base = n - B
        r = [(((int(c[0][k]) << 32) | int(c[1][k])) * (base + k + 1)) >> 64 for k in range(B)]
        first = {}
        dup = []
        for k in range(B):
            dup.append(r[k] in first)
            first.setdefault(r[k], k)
        picks = []
        for k in range(B):
            cur, hit = k, False
            for _ in range(B):
                if dup[cur]:
                    hit = True
                    break
                s = r[cur] - base
                if s < 0 or s >= cur:
                    break
                cur = s
            picks.append(base + k if hit else r[k])
        assert picks == floyd_positions(n, B, 77, d).tolist(), (n, B, d)


def test_entry_points_refuse_bad_arguments_by_name():
    from oac_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int32 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    u64 = ctypes.c_uint64

    def take(len_, B, cap=100, valid_in=p, queue=p, idx=p, out=p, scratch=p, positions=None):
        # out == valid_in is refused too, so a passing call would need distinct buffers;
        # none of these reaches a launch
        return L.oac_replay_nr_take(valid_in, len_, positions, B, queue, cap, 0, idx, None, out,
                                    scratch, u64(1), u64(0), None)

    def err():
        return L.oac_last_error()

    assert take(10, 0) != 0 and b"replay_nr_take" in err() and b"< 1" in err()
    assert take(10, 11) != 0 and b"replay_nr_take" in err() and b"> len" in err()
    assert take(5000, 4097, cap=6000) != 0 and b"replay_nr_take" in err() and b"4096" in err()
    assert take(10, 2, cap=2 ** 31) != 0 and b"replay_nr_take" in err() and b"2^31" in err()
    for kw in ("valid_in", "queue", "idx", "out", "scratch"):
        assert take(10, 2, **{kw: None}) != 0
        assert b"replay_nr_take" in err() and b"null buffer" in err(), kw
    assert take(10, 2) != 0 and b"aliases" in err()

    def draw(n, B, out=p):
        return L.oac_replay_nr_sample_positions(n, B, u64(1), u64(0), out, None)
    assert draw(10, 0) != 0 and b"replay_nr_sample_positions" in err() and b"< 1" in err()
    assert draw(10, 11) != 0 and b"replay_nr_sample_positions" in err() and b"> len" in err()
    assert draw(5000, 4097) != 0 and b"replay_nr_sample_positions" in err() and b"4096" in err()
    assert draw(2 ** 31, 2) != 0 and b"replay_nr_sample_positions" in err() and b"2^31" in err()
    assert draw(10, 2, None) != 0 and b"null buffer" in err()

    def insert(n, len_=0, cap=100, storage=p, queue=p, valid=p, data=p):
        return L.oac_replay_nr_insert(storage, 8, cap, 0, queue, 0, 0, valid, len_, n, data, data,
                                      data, data, data, 2, 1, 0, 2, 3, 4, 5, None)
    assert insert(1, cap=2 ** 31) != 0 and b"replay_nr_insert" in err() and b"2^31" in err()
    for kw in ("storage", "queue", "valid", "data"):
        assert insert(1, **{kw: None}) != 0
        assert b"replay_nr_insert" in err() and b"null buffer" in err(), kw
    assert insert(3, len_=98) != 0 and b"replay_nr_insert" in err() and b"> capacity" in err()
    assert insert(0) == 0, err()      # nothing to do: no launch
    assert L.oac_replay_nr_chunk() == CHUNK
    assert L.oac_abi_version() == 3


def test_the_class_is_exported():
    from oac_amd import ReplayBuffer, ReplayBufferNoResampling
    assert issubclass(ReplayBufferNoResampling, ReplayBuffer)
    for m in ("add_sample", "add_path", "add_paths", "add_indices_to_replace", "random_batch",
              "num_steps_can_sample", "get_diagnostics", "end_epoch", "get_snapshot",
              "restore_from_snapshot", "seed_device_stream", "_take"):
        assert callable(getattr(ReplayBufferNoResampling, m)), m
