"""Generate the ReplayBufferNoResampling fixtures by running the REFERENCE class
(/root/reference/replay_buffer_no_resampling.py) under make_golden.py's harness
(its gym stub): scripted schedules of add_path / random_batch with
``np.random.seed`` set, recording after EVERY operation the drawn indices, the
live list ``_valid_indeces``, the freed-slot ring ``indices_to_replace`` and the
four counters; at the end the five field arrays and one
``np.random.randint(2**31)`` that pins the global stream's position.  The
inserted paths are tests/noresample_oracle.py make_path's, a function of the
recorded ``data_seed`` alone, so the fixtures need not hold them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_noresample.py

Every schedule obeys live + m <= N (the device buffer refuses an insert that
would write over a live row; the reference would wrap onto it).  Runs only
where the read-only reference is present; the .npz files hold inputs and the
states the reference went through on them, nothing else.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the oracle package

from make_golden import Box, save  # noqa: E402  (installs the gym stub, adds the reference)
from replay_buffer_no_resampling import ReplayBufferNoResampling  # noqa: E402
from noresample_oracle import make_path  # noqa: E402  (the paths: a function of data_seed alone)

OBS, ACT = 3, 2


def _state(rb, out, k):
    out[f"op{k}/valid"] = np.asarray([int(i) for i in rb._valid_indeces], np.int32)
    out[f"op{k}/queue"] = rb.indices_to_replace.astype(np.int32)
    out[f"op{k}/counters"] = np.array([rb._top, rb._bottom_indexes, rb._top_indexes, rb._size],
                                      np.int64)


def run(name, N, ops, np_seed, data_seed, snap_at=None):
    """ops: [("add", m) | ("draw", B)].  snap_at: the op after which the
    reference's own get_snapshot is recorded."""
    rb = ReplayBufferNoResampling(N, Box(-1, 1, (OBS,)), Box(-1, 1, (ACT,)))
    rs = np.random.RandomState(data_seed)
    np.random.seed(np_seed)
    out = {}
    for k, (what, n) in enumerate(ops):
        live = len(rb._valid_indeces)
        if what == "add":
            assert live + n <= N, (name, k, live, n)
            rb.add_path(make_path(rs, n, OBS, ACT))
        else:
            assert 1 <= n <= live, (name, k, live, n)
            st = np.random.get_state()
            batch = rb.random_batch(n)
            # the indices: the reference's own draw from the saved stream state
            r2 = np.random.RandomState()
            r2.set_state(st)
            idx = r2.choice(out[f"op{k - 1}/valid"], size=n, replace=False).astype(int)
            assert np.array_equal(batch["observations"], rb._observations[idx])
            assert rb.indices_to_replace[(rb._top_indexes - 1) % N] == idx[-1]
            out[f"op{k}/idx"] = idx.astype(np.int32)
        _state(rb, out, k)
        assert len(set(rb._valid_indeces)) == len(rb._valid_indeces)
        if snap_at == k:
            for key, v in rb.get_snapshot().items():
                out[f"snap/{key}"] = (np.asarray([int(i) for i in v], np.int64)
                                      if key == "_valid_indeces" else np.array(v))
    out["final/observations"] = rb._observations
    out["final/actions"] = rb._actions
    out["final/rewards"] = rb._rewards
    out["final/terminals"] = rb._terminals
    out["final/next_obs"] = rb._next_obs
    out["final/randint"] = np.array(np.random.randint(2 ** 31), np.int64)
    meta = dict(kind="replay_noresample", N=N, obs_dim=OBS, act_dim=ACT, ops=ops, np_seed=np_seed,
                data_seed=data_seed, snap_at=snap_at)
    save(name, meta, out)


def schedule_ops(B=4, steps=20, loops=3):
    """main.py:569-574 scaled down: N = 5 * steps * B, a fill of 4 * steps * B,
    then per loop steps * B new rows (two paths) and `steps` draws of B."""
    per = steps * B
    ops = [("add", per)] * 4
    for _ in range(loops):
        ops += [("add", 30), ("add", per - 30)] + [("draw", B)] * steps
    return 5 * per, ops


def ragged_ops(N=10, seed=5, n_ops=60):
    """Paths of 1..9 rows and draws of 1..7 within the capacity, with a full
    drain of N rows (N freed slots: the ring then reads as empty) and a refill."""
    rs = np.random.RandomState(seed)
    ops, live = [], 0

    def some(n):
        nonlocal live
        for _ in range(n):
            if live and (live == N or rs.uniform() < 0.5):
                b = int(rs.randint(1, min(7, live) + 1))
                ops.append(("draw", b))
                live -= b
            else:
                m = int(rs.randint(1, min(9, N - live) + 1))
                ops.append(("add", m))
                live += m
    some(n_ops // 2)
    while live < N:                       # fill up ...
        m = min(9, N - live)
        ops.append(("add", m))
        live += m
    for b in (7, 3):                      # ... drain all N rows ...
        ops.append(("draw", b))
        live -= b
    assert live == 0
    ops += [("add", 9), ("add", 1)]       # ... and refill
    live = N
    some(n_ops // 2)
    return N, ops


def crossing_ops(N, B=64):
    """List lengths on both sides of N - 1 (256 / 4096): fill, draw below, refill."""
    third = N // 3
    ops = [("add", third), ("add", third), ("add", N - 2 * third)]
    ops += [("draw", B), ("draw", B), ("add", B - 1), ("draw", B), ("add", B + 1), ("add", B),
            ("draw", B), ("draw", 1), ("add", B + 1), ("draw", B)]
    return N, ops


def main():
    N, ops = schedule_ops()
    run("noresample_schedule", N, ops, np_seed=101, data_seed=1)
    N, ops = ragged_ops()
    run("noresample_ragged", N, ops, np_seed=102, data_seed=2)
    N, ops = crossing_ops(257)
    run("noresample_n257", N, ops, np_seed=103, data_seed=3, snap_at=6)
    N, ops = crossing_ops(4097)
    run("noresample_n4097", N, ops, np_seed=104, data_seed=4)


if __name__ == "__main__":
    main()
