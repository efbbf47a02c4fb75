"""oac_amd.ReplayBufferNoResampling on the GPU: the reference's recorded
schedules state by state, the take's compaction at every block edge, the
scatter insert against an ordinary ReplayBuffer's rows, the device position
draw against its CPU restatement bit for bit, the buffer under the one-layer
g-oac / p-oac trainers, snapshots and refusals.  All comparisons are exact
(integers, or float32 bit patterns)."""
import numpy as np
import pytest
import torch

import parity
import shallow_lib as sl
from gpu_helpers import Space
from noresample_oracle import (CHUNK, DRAW_CASES, DRAW_COUNTERS, GOLDENS, TAKE_LENGTHS,
                               NoResampleOracle, floyd_positions, make_path, take_cases)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _buffer(N, Do=3, Da=2, **kw):
    from oac_amd import ReplayBufferNoResampling
    return ReplayBufferNoResampling(N, Space(Do), Space(Da), device=DEV, **kw)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _state(rb):
    """(list, ring, [top, bottom, top_indexes, size]) downloaded."""
    return (_host(rb.valid_indices()).astype(np.int64), _host(rb._queue).astype(np.int64),
            [rb._top, rb._bottom_indexes, rb._top_indexes, rb._size])


def _check_golden_state(rb, g, k, what):
    lst, ring, counters = _state(rb)
    np.testing.assert_array_equal(lst, g[f"op{k}/valid"], err_msg=f"{what}: list")
    np.testing.assert_array_equal(ring, g[f"op{k}/queue"], err_msg=f"{what}: ring")
    assert counters == g[f"op{k}/counters"].tolist(), what
    assert rb.num_steps_can_sample() == counters[3] and rb._live == len(lst), what


def _rows_of(rb, obs, act, rew, term, nobs):
    """float64 field arrays [N, .] as the float32 rows of the device store."""
    r = rb.rows
    want = np.zeros((len(obs), r["row_stride"]), np.float32)
    want[:, r["off_obs"]:r["off_obs"] + rb.ob_dim] = np.float32(obs)
    want[:, r["off_act"]:r["off_act"] + rb.ac_dim] = np.float32(act)
    want[:, r["off_rew"]] = np.float32(np.asarray(rew)[:, 0])
    want[:, r["off_term"]] = np.asarray(term)[:, 0].astype(np.float32)
    want[:, r["off_next_obs"]:r["off_next_obs"] + rb.ob_dim] = np.float32(nobs)
    return want


def _run_ops(rb, meta, g, rs, first, last):
    for k in range(first, last):
        what, n = meta["ops"][k]
        if what == "add":
            rb.add_path(make_path(rs, n, meta["obs_dim"], meta["act_dim"]))
        else:
            batch = rb.random_batch(n)
            assert batch.indices.dtype == torch.int32 and batch.indices.is_cuda
            np.testing.assert_array_equal(_host(batch.indices), g[f"op{k}/idx"],
                                          err_msg=f"op {k}: drawn slots")
        _check_golden_state(rb, g, k, f"op {k} ({what} {n})")


# ---------------------------------------------------------- 1. golden schedules
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_schedule_state_by_state(name):
    meta, g = parity.load(name)
    rb = _buffer(meta["N"], meta["obs_dim"], meta["act_dim"], index_source="numpy")
    rs = np.random.RandomState(meta["data_seed"])
    np.random.seed(meta["np_seed"])
    _run_ops(rb, meta, g, rs, 0, len(meta["ops"]))
    want = _rows_of(rb, g["final/observations"], g["final/actions"], g["final/rewards"],
                    g["final/terminals"], g["final/next_obs"])
    np.testing.assert_array_equal(_host(rb._storage).view(np.uint32), want.view(np.uint32))
    assert np.random.randint(2 ** 31) == int(g["final/randint"])


# ------------------------------------------------------- 2. compaction edges
@pytest.mark.parametrize("n", TAKE_LENGTHS)
def test_take_equals_np_delete_at_every_edge(n):
    from oac_amd import _lib
    assert _lib.lib().oac_replay_nr_chunk() == CHUNK
    N = n + 3
    rb = _buffer(N, 1, 1)
    cases = [c for c in take_cases() if c[1] == n]
    assert cases
    lst = np.random.RandomState(n).permutation(N)[:n].astype(np.int32)
    for name, _, pos in cases:
        B = len(pos)
        cur = rb._cur
        rb._valid[cur].fill_(-9)
        rb._valid[cur][:n].copy_(torch.from_numpy(lst))
        rb._valid[1 - cur].fill_(-7)          # the other buffer: poison everywhere
        rb._queue.fill_(-5)
        rb._live = rb._size = n
        rb._top_indexes = rb._bottom_indexes = N - 2    # the ring wraps for B >= 3
        got = _host(rb._take(pos))
        np.testing.assert_array_equal(got, lst[pos], err_msg=f"{name}: slots")
        assert rb._cur == 1 - cur and rb._live == n - B and rb._size == n - B, name
        out = _host(rb._valid[rb._cur])
        np.testing.assert_array_equal(out[:n - B], np.delete(lst, pos), err_msg=f"{name}: list")
        assert (out[n - B:] == -7).all(), f"{name}: wrote past the new list"
        ring = _host(rb._queue)
        at = (N - 2 + np.arange(B)) % N
        np.testing.assert_array_equal(ring[at], lst[pos], err_msg=f"{name}: ring")
        rest = np.ones(N, bool)
        rest[at] = False
        assert (ring[rest] == -5).all(), f"{name}: ring entries not written changed"
        assert rb._top_indexes == (N - 2 + B) % N, name
        np.testing.assert_array_equal(_host(rb._valid[cur])[:n], lst, err_msg=f"{name}: source")


def test_take_refuses_bad_positions():
    rb = _buffer(16, 1, 1)
    rb.add_path(make_path(np.random.RandomState(0), 8, 1, 1))
    before = _state(rb)
    for bad in ([0, 0], [8], [-1], []):
        with pytest.raises(ValueError):
            rb._take(np.asarray(bad, np.int64))
    after = _state(rb)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---------------------------------------------------------- 3. scatter insert
def test_scatter_insert_equals_an_ordinary_insert_at_the_same_slots():
    from oac_amd import ReplayBuffer
    N, Do, Da, q = 400, 3, 2, 40
    rs = np.random.RandomState(5)
    ring_slots = (300 + rs.permutation(90)[:q]).astype(np.int32)   # disjoint from the _top run
    live0 = np.arange(390, 394, dtype=np.int32)
    bottom, top = N - 10, N - 5                                    # both wrap
    for m in (0, 1, q - 1, q, q + 1, q + 300):
        rb = _buffer(N, Do, Da)
        rb._storage.fill_(-123.0)
        rb._valid[rb._cur].fill_(-9)
        rb._valid[rb._cur][:len(live0)].copy_(torch.from_numpy(live0))
        rb._live = rb._size = len(live0)
        ring = np.full(N, -5, np.int32)
        ring[(bottom + np.arange(q)) % N] = ring_slots
        rb._queue.copy_(torch.from_numpy(ring))
        rb._bottom_indexes, rb._top_indexes, rb._top = bottom, (bottom + q) % N, top
        path = make_path(rs, m, Do, Da)
        rb.add_path(path)
        k = min(m, q)
        slots = np.concatenate([ring_slots[:k], (top + np.arange(m - k)) % N]).astype(np.int64)
        assert len(set(slots.tolist())) == m
        what = f"m={m}"
        assert [rb._top, rb._bottom_indexes, rb._top_indexes, rb._size, rb._live] == \
            [(top + m - k) % N, (bottom + k) % N, (bottom + q) % N, len(live0) + m,
             len(live0) + m], what
        lst = _host(rb._valid[rb._cur])
        np.testing.assert_array_equal(lst[:len(live0) + m], np.concatenate([live0, slots]),
                                      err_msg=what)
        assert (lst[len(live0) + m:] == -9).all(), what
        np.testing.assert_array_equal(_host(rb._queue), ring, err_msg=f"{what}: ring")
        got = _host(rb._storage)
        want = np.full_like(got, -123.0)
        if m:
            plain = ReplayBuffer(N, Space(Do), Space(Da), device=DEV)
            plain.add_path(path)
            want[slots] = _host(plain._storage)[:m]
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)
        if m:
            assert not got[slots][:, rb.rows["off_next_obs"] + Do:].any(), f"{what}: pad columns"


def test_add_sample_one_by_one_equals_add_path():
    a, b = _buffer(32), _buffer(32)
    rs = np.random.RandomState(1)
    for n, B in ((9, 4), (6, 5), (7, 3)):
        path = make_path(rs, n, 3, 2)
        a.add_path(path)
        for i in range(n):
            b.add_sample(path["observations"][i], path["actions"][i], path["rewards"][i],
                         path["next_observations"][i], path["terminals"][i], env_info={})
        pos = rs.permutation(a._live)[:B]
        assert np.array_equal(_host(a._take(pos)), _host(b._take(pos)))
    assert torch.equal(a._storage, b._storage)
    sa, sb = _state(a), _state(b)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert a.get_diagnostics()["size"] == a._size and a.end_epoch(0) is None


# -------------------------------------------------------------- 4. device draw
@pytest.mark.parametrize("n,B", DRAW_CASES)
def test_device_draw_equals_the_restatement(n, B):
    rb = _buffer(8, 1, 1, index_source="device", seed=0x1234_5678_9ABC)
    for d in DRAW_COUNTERS:
        got = _host(rb.sample_positions_device(n, B, draw_counter=d)).astype(np.int64)
        np.testing.assert_array_equal(got, floyd_positions(n, B, 0x1234_5678_9ABC, d),
                                      err_msg=f"counter {d}")
    assert rb._draws == 0


def test_device_random_batch_counter_and_seed():
    seed, N = 99, 300
    bufs = [_buffer(N, 1, 1, index_source="device", seed=seed) for _ in range(2)]
    path = make_path(np.random.RandomState(2), 200, 1, 1)
    for rb in bufs:
        rb.add_path(path)
    orc = NoResampleOracle(N)
    orc.add(200)
    state0 = np.random.get_state()[1].copy()
    for d, B in enumerate((32, 1, 64)):
        got = [_host(rb.random_batch(B).indices).astype(np.int64) for rb in bufs]
        want = orc.take(floyd_positions(len(orc.valid), B, seed, d))
        np.testing.assert_array_equal(got[0], want, err_msg=f"draw {d}")
        np.testing.assert_array_equal(got[1], want)
        assert bufs[0]._draws == d + 1
        np.testing.assert_array_equal(_state(bufs[0])[0], orc.valid)
    assert np.array_equal(np.random.get_state()[1], state0), "the device draw uses no host numbers"
    rb = bufs[0]
    rb.seed_device_stream(seed)                 # restarts the counter
    assert rb._draws == 0
    got = _host(rb.random_batch(16).indices).astype(np.int64)
    np.testing.assert_array_equal(got, orc.valid[floyd_positions(len(orc.valid), 16, seed, 0)])


# --------------------------------------------------------- 5. through a trainer
def _tstate(tr):
    torch.cuda.synchronize()
    return torch.cat([tr.params, tr.targets, tr.adam_m, tr.adam_v]).cpu().numpy()


@pytest.mark.parametrize("fixture", ["goac_d1_plain", "ptrain_d1_plain"])
def test_trainer_steps_equal_an_ordinary_buffers_batches(fixture):
    from oac_amd import DeviceBatch, ReplayBuffer
    meta, _ = parity.load(fixture)
    assert meta["hidden"] == [16]
    Do, Da, N, B = meta["obs_dim"], meta["act_dim"], 200, 32
    path = make_path(np.random.RandomState(3), N, Do, Da)
    nr = _buffer(N, Do, Da, index_source="device", seed=5)
    plain = ReplayBuffer(N, Space(Do), Space(Da), device=DEV)
    nr.add_path(path)
    plain.add_path(path)
    assert torch.equal(nr._storage, plain._storage)
    tr_a, tr_b = sl.trainer_for(meta), sl.trainer_for(meta)
    drawn = []
    for _ in range(3):
        batch = nr.random_batch(B)
        batch["buffer"] = nr
        idx = batch.indices.clone()
        drawn.append(_host(idx))
        tr_a.train(batch)
        other = DeviceBatch(plain, idx)
        other["buffer"] = plain
        tr_b.train(other)
    a, b = _tstate(tr_a), _tstate(tr_b)
    assert np.isfinite(a).all()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert len(set(np.concatenate(drawn).tolist())) == 3 * B
    # a key read from the batch gathers that field of the drawn rows
    batch = nr.random_batch(4)
    r = nr.rows
    rows = _host(nr._storage)[_host(batch.indices)]
    np.testing.assert_array_equal(_host(batch["rewards"]), rows[:, r["off_rew"]:r["off_rew"] + 1])


def test_device_schedule_draws_every_row_once_per_residence():
    meta, _ = parity.load("noresample_schedule")
    N, Do, Da = meta["N"], meta["obs_dim"], meta["act_dim"]
    rb = _buffer(N, Do, Da, index_source="device", seed=7)
    orc = NoResampleOracle(N)
    rs = np.random.RandomState(11)
    resident = {}            # slot -> float32 reward of the row living there
    inserted = drawn = 0
    for what, n in meta["ops"]:
        if what == "add":
            path = make_path(rs, n, Do, Da)
            rb.add_path(path)
            slots = orc.add(n)
            for s, rew in zip(slots.tolist(), np.float32(path["rewards"][:, 0])):
                assert s not in resident, "an insert wrote over a live row"
                resident[s] = rew
            inserted += n
        else:
            batch = rb.random_batch(n)
            idx = _host(batch.indices).astype(np.int64)
            rew = _host(batch["rewards"])[:, 0]
            assert len(set(idx.tolist())) == n
            for s, x in zip(idx.tolist(), rew):
                assert s in resident, "a freed slot was drawn"
                assert resident.pop(s) == x
            where = {v: i for i, v in enumerate(orc.valid.tolist())}
            orc.take([where[s] for s in idx.tolist()])
            drawn += n
        lst, ring, counters = _state(rb)
        np.testing.assert_array_equal(lst, orc.valid)
        np.testing.assert_array_equal(ring, orc.queue.astype(np.int64))
        assert counters == orc.counters()
        assert sorted(resident) == sorted(lst.tolist())
    assert (inserted, drawn) == (4 * 80 + 3 * 80, 3 * 80) and len(resident) == inserted - drawn


# ------------------------------------------------- 6. snapshots and refusals
def test_snapshot_round_trip_and_the_references_snapshot():
    meta, g = parity.load("noresample_n257")
    N, Do, Da, at = meta["N"], meta["obs_dim"], meta["act_dim"], meta["snap_at"]
    # the reference's own snapshot, then the golden's next states
    ss = {k[5:]: g[k] for k in g if k.startswith("snap/")}
    assert len(ss) == 11
    for k in ("_top", "_bottom_indexes", "_top_indexes", "_size"):
        ss[k] = int(ss[k])
    ss["_valid_indeces"] = ss["_valid_indeces"].tolist()
    rb = _buffer(N, Do, Da)
    rb.restore_from_snapshot(ss)
    _check_golden_state(rb, g, at, "restored")
    rs = np.random.RandomState(meta["data_seed"])
    np.random.seed(meta["np_seed"])
    live = 0
    for what, n in meta["ops"][:at + 1]:        # the two host streams up to the snapshot
        if what == "add":
            make_path(rs, n, Do, Da)
            live += n
        else:
            np.random.choice(live, size=n, replace=False)
            live -= n
    _run_ops(rb, meta, g, rs, at + 1, len(meta["ops"]))
    want = _rows_of(rb, g["final/observations"], g["final/actions"], g["final/rewards"],
                    g["final/terminals"], g["final/next_obs"])
    np.testing.assert_array_equal(_host(rb._storage).view(np.uint32), want.view(np.uint32))
    # round trip: the reference's eleven keys and dtypes
    snap = rb.get_snapshot()
    assert sorted(snap) == sorted(rb.SNAPSHOT_KEYS) and len(snap) == 11
    last = len(meta["ops"]) - 1
    assert snap["_indices_to_replace"].dtype == np.uint64
    np.testing.assert_array_equal(snap["_indices_to_replace"],
                                  g[f"op{last}/queue"].astype(np.uint64))
    assert all(type(i) is int for i in snap["_valid_indeces"])
    assert snap["_valid_indeces"] == g[f"op{last}/valid"].tolist()
    assert snap["_observations"].dtype == np.float64 and snap["_terminals"].dtype == np.uint8
    assert snap["_observations"].shape == (N, Do) and snap["_rewards"].shape == (N, 1)
    rb2 = _buffer(N, Do, Da)
    rb2.restore_from_snapshot(snap)
    assert torch.equal(rb2._storage, rb._storage)
    s1, s2 = _state(rb), _state(rb2)
    assert all(np.array_equal(x, y) for x, y in zip(s1, s2))
    np.random.seed(1)
    a = _host(rb.random_batch(7).indices)
    np.random.seed(1)
    b = _host(rb2.random_batch(7).indices)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("source", ["numpy", "device"])
def test_refusals_by_name_leave_the_state_unchanged(source):
    N = 20
    rb = _buffer(N, index_source=source, seed=3)
    rs = np.random.RandomState(0)
    rb.add_path(make_path(rs, 15, 3, 2))
    rb.random_batch(5)
    rb.add_path(make_path(rs, 2, 3, 2))

    def full():
        return _state(rb) + (_host(rb._storage).copy(), rb._live, rb._draws)
    before = full()
    np.random.seed(4)
    stream = np.random.get_state()[1].copy()
    with pytest.raises(RuntimeError) as e:       # 12 live + 9 > 20
        rb.add_path(make_path(rs, 9, 3, 2))
    msg = str(e.value)
    assert "ReplayBufferNoResampling" in msg and "12" in msg and "9" in msg and "20" in msg
    with pytest.raises(ValueError) as e:
        rb.random_batch(13)
    with pytest.raises(ValueError) as ref:
        np.random.choice(12, size=13, replace=False)
    assert str(e.value) == str(ref.value)
    with pytest.raises(NotImplementedError, match="ReplayBufferNoResampling"):
        rb.get_dataset()
    after = full()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert np.array_equal(np.random.get_state()[1], stream)
    rb.add_path(make_path(rs, 8, 3, 2))          # exactly the capacity is fine
    assert rb._live == N and rb.num_steps_can_sample() == N
