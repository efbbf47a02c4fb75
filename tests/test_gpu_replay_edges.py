"""The replay side on the device at the edges of tests/replay_cases.py:
priority sampling (csrc/replay_count.hip prio_scan_blocks / prio_scan_tops /
prio_search) at every scan edge, the counts bookkeeping across its block and
loop edges and across the host and device epochs, the device index stream
through its ring refills (alone, under SACTrainer, and from a nonzero batch
counter), the MT19937 draws at the ends of a 624-word block and in the
unmasked branch, and the insert / gather kernels at their row and batch edges.

Every assertion is an exact equality against numpy or oracle/replay_oracle.py
(tests/test_replay_cases_cpu.py asserts what makes that well defined)."""
import ctypes

import numpy as np
import pytest
import torch

import replay_cases as rc
from fixtures_lib import sac_params, synthetic_transitions
from gpu_helpers import Space, producers
from oracle.replay_oracle import CountReplayOracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from oac_amd import _lib as L
    return L


# ------------------------------------------------------ 1. priority sampling
def _priority_abi(counts_dev, size, u, capacity=None):
    """oac_replay_priority_sample for hand-built uniforms; the scratch sized by
    oac_replay_priority_scratch_doubles and fenced with NaN so that a read of
    an unwritten prefix cannot pass for a weight."""
    L = _lib()
    n = int(L.lib().oac_replay_priority_scratch_doubles(capacity or size))
    scratch = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    ud = torch.tensor(u, dtype=torch.float64, device=DEV)
    out = torch.full((len(u),), -7, dtype=torch.int32, device=DEV)
    L.check(L.lib().oac_replay_priority_sample(L.ptr(counts_dev), size, L.ptr(ud), len(u),
                                               L.ptr(scratch), L.ptr(out), L.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name", [c.name for c in rc.DYADIC if c.size == c.capacity])
def test_priority_dyadic_rows_exact_for_every_u(name):
    c = rc.DYADIC_BY_NAME[name]
    counts, u, want, tie = rc.dyadic_reference(c)
    got = _priority_abi(torch.tensor(counts).to(DEV), c.size, u)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, [(int(i), float(u[i]), int(got[i]), int(want[i])) for i in bad[:8]])


def test_priority_size_below_capacity_through_the_buffer():
    """4097 valid rows in a buffer of 10,000: the ABI call with hand-built u
    and ReplayBufferCount._priority_indices (numpy's own random_sample draws)
    on the same buffer; rows past the size are never read."""
    from oac_amd import ReplayBufferCount
    c = rc.DYADIC_BY_NAME["dyadic-4097-of-10000"]
    counts, u, want, _tie = rc.dyadic_reference(c)
    rb = ReplayBufferCount(c.capacity, Space(1), Space(1), priority_sample=True, device=DEV)
    rb._size, rb._top = c.size, c.size
    rb._counts.copy_(torch.tensor(counts))
    got = _priority_abi(rb._counts, rb._size, u, capacity=c.capacity)
    np.testing.assert_array_equal(got, want)
    np.random.seed(31)
    got = rb._priority_indices(777).cpu().numpy()
    u2 = np.random.RandomState(31).random_sample(777)
    np.testing.assert_array_equal(got, rc.oracle_indices(counts[:c.size], u2))
    assert got.max() < c.size


@pytest.mark.parametrize("name", [c.name for c in rc.GENERAL])
def test_priority_general_rows_equal_numpy(name):
    from oac_amd import ReplayBufferCount
    c = rc.GENERAL_BY_NAME[name]
    counts, u, want = rc.general_reference(c)
    rb = ReplayBufferCount(c.size, Space(1), Space(1), priority_sample=True, device=DEV)
    rb._size = c.size
    rb._counts.copy_(torch.tensor(counts))
    np.random.seed(c.seed + 1)
    got = rb._priority_indices(c.B).cpu().numpy().astype(np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, [(int(i), float(u[i]), int(got[i]), int(want[i])) for i in bad[:8]])


def test_priority_abi_bounds():
    L = _lib()
    counts = torch.zeros(8, dtype=torch.int32, device=DEV)
    u = torch.full((4,), 0.5, dtype=torch.float64, device=DEV)
    scratch = torch.zeros(64, dtype=torch.float64, device=DEV)
    out = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    args = lambda size, B: (L.ptr(counts), size, L.ptr(u), B, L.ptr(scratch), L.ptr(out),
                            L.stream_ptr())
    for size in (0, rc.MAX_SIZE + 1):
        assert L.lib().oac_replay_priority_sample(*args(size, 4)) != 0
        assert b"priority sample: size must be in [1, 4194304]" in L.lib().oac_last_error()
    assert L.lib().oac_replay_priority_sample(*args(8, 0)) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all() and not scratch.cpu().numpy().any()


# -------------------------------------------------------- 2. counts bookkeeping
def _small_count_buffer(n=rc.COUNT_ROWS, Do=3, Da=2, **kw):
    from oac_amd import ReplayBufferCount
    rb = ReplayBufferCount(n, Space(Do), Space(Da), device=DEV, **kw)
    rb.load_transitions(torch.zeros(n, rb.rows["row_stride"], device=DEV))
    return rb


def _tiny_path(rs, n, Do=3, Da=2):
    return dict(observations=rs.standard_normal((n, Do)), actions=rs.standard_normal((n, Da)),
                rewards=rs.standard_normal((n, 1)), next_observations=rs.standard_normal((n, Do)),
                terminals=rs.randint(0, 2, (n, 1)).astype(np.uint8))


@pytest.mark.parametrize("B", rc.COUNT_BATCHES)
def test_counts_update_equals_numpy_fancy_increment(B):
    """50 rows, so every batch past 50 is full of duplicates, within and
    across the 256-thread blocks; several calls (the epoch advances), a path
    inserted in between (its rows' counts reset, their tags stay stale)."""
    rb = _small_count_buffer()
    orc = CountReplayOracle(rc.COUNT_ROWS, 3, 2)
    orc.size = rc.COUNT_ROWS
    np.random.seed(B)
    ref = []
    for call in range(5):
        if call == 2:
            orc.add_path(_tiny_path(np.random.RandomState(9), 7))
        batch, idx, _ = orc.random_batch(B)
        ref.append((idx, batch["counts"][:, 0].copy(), orc.counts[:, 0].copy()))
    np.random.seed(B)
    for call, (idx, before, after) in enumerate(ref):
        if call == 2:
            rb.add_path(_tiny_path(np.random.RandomState(9), 7))
        batch = rb.random_batch(B)
        what = f"B={B} call {call}"
        np.testing.assert_array_equal(batch.indices.cpu().numpy(), idx, err_msg=what)
        np.testing.assert_array_equal(batch["counts"].cpu().numpy()[:, 0], before.astype(np.float32),
                                      err_msg=what)
        np.testing.assert_array_equal(rb._counts.cpu().numpy(), after.astype(np.int32), err_msg=what)
    assert rb._epoch == 5
    assert B < rc.COUNT_ROWS or len(np.unique(ref[0][0])) < B   # duplicates in the batch


def _ring_counts_run(B, chunk, phases, seed=4):
    """Host random_batch calls, ring steps and host calls again on one
    300-row buffer (test_gpu_ring's counts buffer and g-oac trainer): the
    batch counts of every step and the counts array after it against
    ``c[idx] += 1``.  phases: [("host", calls) | ("ring", steps)]."""
    from oac_amd import DeviceIndexStream
    from test_gpu_ring import _count_buffer, _counts_trainer
    rb = _count_buffer()
    assert rb._size == rc.RING_COUNT_ROWS
    tr = _counts_trainer("goac")
    want = np.zeros(rc.RING_COUNT_ROWS, np.int64)
    for k, (kind, n) in enumerate(phases):
        draws = rc.stream_draws(seed + k, n, size=rc.RING_COUNT_ROWS, B=B)
        if kind == "host":
            rb.seed_device_stream(seed + k)
            for j, idx in enumerate(draws):
                batch = rb.random_batch(B)
                before = rc.bump(want, idx)
                what = f"phase {k} host call {j}"
                np.testing.assert_array_equal(batch.indices.cpu().numpy(), idx, err_msg=what)
                np.testing.assert_array_equal(batch["counts"].cpu().numpy()[:, 0],
                                              before.astype(np.float32), err_msg=what)
                np.testing.assert_array_equal(rb._counts.cpu().numpy(), want, err_msg=what)
        else:
            st = DeviceIndexStream(rb, B, chunk=chunk, seed=seed + k,
                                   start=int(tr.step_state[1].item()))
            for j, idx in enumerate(draws):
                st.before_step(1)
                tr.train_from_ring(rb._storage, st.ring, st.slots, B, n_steps=1,
                                   count_state=rb.device_count_state())
                torch.cuda.synchronize()
                before = rc.bump(want, idx)
                what = f"phase {k} ring step {j}"
                got = tr._last_plan.views["counts"].cpu().numpy().reshape(-1)
                np.testing.assert_array_equal(got, before.astype(np.float32), err_msg=what)
                np.testing.assert_array_equal(rb._counts.cpu().numpy(), want, err_msg=what)
    assert torch.isfinite(tr.params).all()
    return rb


def test_counts_host_and_device_epochs_alternate_on_one_buffer():
    rb = _ring_counts_run(32, 2, [("host", 3), ("ring", 9), ("host", 3), ("ring", 5), ("host", 2)])
    assert rb._epoch == 8 and int(rb._epoch_dev.item()) == (1 << 30) + 14


def test_counts_ring_step_past_1024_rows_loops_over_the_batch():
    """B = 1025: the smallest batch past counts_step_kernel's 1024 threads (the
    step admits it; its loop over the batch runs a second pass of one row)."""
    _ring_counts_run(1025, 2, [("host", 1), ("ring", 5), ("host", 1)])


# ------------------------------------------- 3. index stream and ring refill
def _stream_buffer(Do=7, Da=5, n=rc.STREAM_ROWS):
    """Replay row r holds float(r) in obs column 0 (exact in float32)."""
    from oac_amd import ReplayBuffer
    rb = ReplayBuffer(n, Space(Do), Space(Da), device=DEV)
    d = synthetic_transitions(n, Do, Da, seed=1)
    rows = rb._rows_from(d["observations"], d["actions"], d["rewards"], d["next_observations"],
                         d["terminals"])
    rows[:, rb.rows["off_obs"]] = np.arange(n, dtype=np.float32)
    rb.load_transitions(torch.from_numpy(rows).to(DEV))
    return rb


def _sac_trainer(Do=7, Da=5, H=32):
    from oac_amd import SACTrainer
    pp, qp = producers(sac_params(Do, Da, [H, H], 3, pi_init_w=0.2, q_init_w=0.1))
    return SACTrainer(pp, qp, action_space=Space(Da), discount=0.99, reward_scale=1.0,
                      policy_lr=1e-3, qf_lr=1e-3, soft_target_tau=5e-3,
                      use_automatic_entropy_tuning=True, device=DEV, seed=7)


@pytest.mark.parametrize("start", [0, 3, rc.STREAM_CHUNK + 2, 2 * rc.STREAM_CHUNK + 1],
                         ids=lambda s: f"start{s}")
def test_index_stream_slots_equal_numpy_through_the_refills(start):
    """The stream alone: before every block of 1, 2 or 4 steps the slots the
    block will consume, (start + t) % slots, hold numpy's draws of those steps
    -- through five refills, every refilled half read back."""
    from oac_amd import DeviceIndexStream, ReplayBuffer
    rb = ReplayBuffer(rc.STREAM_ROWS, Space(1), Space(1), device=DEV)
    rb._size = rc.STREAM_ROWS
    B, chunk, seed = rc.STREAM_B, rc.STREAM_CHUNK, 21
    st = DeviceIndexStream(rb, B, chunk=chunk, seed=seed, start=start)
    assert st.slots == 2 * chunk
    draws = rc.stream_draws(seed, sum(rc.STREAM_BLOCKS))
    t = 0
    for n in rc.STREAM_BLOCKS:
        st.before_step(n)
        ring = st.ring.cpu().numpy().reshape(st.slots, B)
        for k in range(t, t + n):
            np.testing.assert_array_equal(ring[(start + k) % st.slots], draws[k],
                                          err_msg=f"stream step {k} (block of {n})")
        t += n
    assert st.t == t == 6 * chunk


def _advance(tr, rb, steps, B):
    """Gradient steps on another path (the synchronous device-index one)."""
    from oac_amd.replay_buffer import DeviceBatch
    tr._no_dropin = True
    rs = np.random.RandomState(99)
    for _ in range(steps):
        tr.train(DeviceBatch(rb, host_indices=rs.randint(0, rb._size, B)))
    torch.cuda.synchronize()
    assert int(tr.step_state[1].item()) == steps


@pytest.mark.parametrize("offset", [0, 5, rc.STREAM_CHUNK + 2], ids=lambda s: f"bc{s}")
def test_ring_steps_gather_numpys_draws(offset):
    """SACTrainer at (7, 5, 32), B = 37, single ring steps across 5 chunks:
    after each step obs column 0 of the plan's batch is that step's numpy
    draw.  The trainer first takes ``offset`` steps on another path; the stream
    is attached at its batch counter (start=)."""
    from oac_amd import DeviceIndexStream
    rb, tr = _stream_buffer(), _sac_trainer()
    B, chunk, seed = rc.STREAM_B, rc.STREAM_CHUNK, 22
    _advance(tr, rb, offset, B)
    st = DeviceIndexStream(rb, B, chunk=chunk, seed=seed, start=int(tr.step_state[1].item()))
    col = rb.rows["off_obs"]
    for k, idx in enumerate(rc.stream_draws(seed, 5 * chunk)):
        st.before_step(1)
        tr.train_from_ring(rb._storage, st.ring, st.slots, B, n_steps=1)
        torch.cuda.synchronize()
        got = tr._last_plan.views["batch"][:, col].cpu().numpy()
        np.testing.assert_array_equal(got, idx.astype(np.float32), err_msg=f"ring step {k}")
    assert torch.isfinite(tr.params).all()


def test_index_stream_refuses_a_negative_start():
    from oac_amd import DeviceIndexStream, ReplayBuffer
    rb = ReplayBuffer(8, Space(1), Space(1), device=DEV)
    rb._size = 8
    with pytest.raises(ValueError, match="start"):
        DeviceIndexStream(rb, 4, chunk=2, seed=1, start=-1)


@pytest.mark.parametrize("offset", [0, rc.STREAM_CHUNK + 2], ids=lambda s: f"bc{s}")
def test_ring_chunk_calls_equal_the_synchronous_index_path(offset):
    """n_steps = chunk ring calls across 5 chunks against tr.train(DeviceBatch(
    rb, host_indices=numpy's draw)) with the drop-in path off: parameters,
    targets, Adam moments and the alpha state bitwise (both draw the Philox
    eps from the same batch counter)."""
    from oac_amd import DeviceIndexStream
    from oac_amd.replay_buffer import DeviceBatch
    B, chunk, seed = rc.STREAM_B, rc.STREAM_CHUNK, 23
    rb_a, tr_a = _stream_buffer(), _sac_trainer()
    _advance(tr_a, rb_a, offset, B)
    st = DeviceIndexStream(rb_a, B, chunk=chunk, seed=seed, start=offset)
    for _ in range(5):
        st.before_step(chunk)
        tr_a.train_from_ring(rb_a._storage, st.ring, st.slots, B, n_steps=chunk)
    rb_b, tr_b = _stream_buffer(), _sac_trainer()
    _advance(tr_b, rb_b, offset, B)
    for idx in rc.stream_draws(seed, 5 * chunk):
        tr_b.train(DeviceBatch(rb_b, host_indices=idx))
    torch.cuda.synchronize()
    assert int(tr_a.step_state[1].item()) == int(tr_b.step_state[1].item()) == offset + 5 * chunk
    for name in ("params", "targets", "adam_m", "adam_v", "alpha_state"):
        a, b = getattr(tr_a, name).cpu().numpy(), getattr(tr_b, name).cpu().numpy()
        if name == "alpha_state":   # log alpha and its Adam state (test_gpu_dropin's _state)
            a, b = a[:4], b[:4]
        assert np.isfinite(a).all(), name
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=name)


# ------------------------------------------------------------------ 4. MT19937
def _mt_buffer(seed, size):
    from oac_amd import ReplayBuffer
    rb = ReplayBuffer(4, Space(1), Space(1), device=DEV)
    rb.seed_device_stream(seed)
    rb._size = size
    return rb


def _draw(rb, n):
    """n device draws as numpy's int64 values, with a fence behind them."""
    out = torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
    rb.sample_indices_device(n, out=out[:n])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == -7).all(), "wrote past count"
    return got[:n].astype(np.int64) & 0xffffffff


@pytest.mark.parametrize("size", rc.MT_SEQUENCE_SIZES)
def test_randint_calls_at_the_ends_of_a_624_word_block(size):
    seed = 77
    rb = _mt_buffer(seed, size)
    for k, want in enumerate(rc.randint_calls(seed, size, rc.MT_COUNTS)):
        np.testing.assert_array_equal(_draw(rb, len(want)), want,
                                      err_msg=f"call {k} of {len(want)} draws")


@pytest.mark.parametrize("size", rc.MT_SINGLE_SIZES)
def test_randint_single_call_at_mask_edges(size):
    seed = 78
    rb = _mt_buffer(seed, size)
    want = np.random.RandomState(seed).randint(0, size, rc.MT_SINGLE_COUNT)
    np.testing.assert_array_equal(_draw(rb, rc.MT_SINGLE_COUNT), want)


def test_randint_unmasked_branch_carries_its_state():
    seed, size = 79, 1 << 32
    rb = _mt_buffer(seed, size)
    for k, want in enumerate(rc.randint_calls(seed, size, (700, 700))):
        assert want.max() >= 1 << 31
        np.testing.assert_array_equal(_draw(rb, 700), want, err_msg=f"call {k}")


def test_randint_size_bounds():
    L = _lib()
    rb = _mt_buffer(1, 10)
    out = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    state = rb._mt.clone()
    for size in (0, (1 << 32) + 1):
        assert L.lib().oac_replay_sample_indices(L.ptr(rb._mt), ctypes.c_uint64(size), 4, L.ptr(out),
                                                 L.stream_ptr()) != 0
        assert b"size must be in [1, 2^32]" in L.lib().oac_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all() and torch.equal(state, rb._mt)


# ------------------------------------------------------- 5. insert and gather
def _wide_path(rs, n, Do, Da):
    f = lambda *shape: rs.standard_normal(shape) * np.pi   # no float64 here is a float32
    return dict(observations=f(n, Do), actions=f(n, Da), rewards=f(n, 1),
                next_observations=f(n, Do), terminals=rs.randint(0, 2, (n, 1)).astype(np.uint8))


def _expected_rows(rb, orc, Do, Da):
    r = rb.rows
    want = np.zeros((orc.N, r["row_stride"]), np.float32)
    want[:, r["off_obs"]:r["off_obs"] + Do] = np.float32(orc.obs)
    want[:, r["off_act"]:r["off_act"] + Da] = np.float32(orc.act)
    want[:, r["off_rew"]] = np.float32(orc.rew[:, 0])
    want[:, r["off_term"]] = orc.term[:, 0].astype(np.float32)
    want[:, r["off_next_obs"]:r["off_next_obs"] + Do] = np.float32(orc.next_obs)
    return want


@pytest.mark.parametrize("Do,Da", rc.INSERT_SHAPES, ids=lambda v: str(v))
def test_insert_rows_without_padding_and_wider_than_a_block(Do, Da):
    from oac_amd import ReplayBuffer
    N = rc.INSERT_CAPACITY
    rb = ReplayBuffer(N, Space(Do), Space(Da), device=DEV)
    orc = CountReplayOracle(N, Do, Da)
    used = rb.rows["off_next_obs"] + Do
    assert rb.rows["row_stride"] - used == (1 if Do == 376 else 0)
    rs = np.random.RandomState(3)
    for step, n in enumerate(rc.INSERT_LENGTHS):
        path = _wide_path(rs, n, Do, Da)
        top0 = rb._top
        before = rb._storage.cpu().numpy().copy()
        rb.add_path(path)
        orc.add_path(path)
        torch.cuda.synchronize()
        got = rb._storage.cpu().numpy()
        what = f"insert {step} (n={n}, top {top0})"
        assert (rb._top, rb._size) == (orc.top, orc.size), what
        np.testing.assert_array_equal(got.view(np.uint32),
                                      _expected_rows(rb, orc, Do, Da).view(np.uint32), err_msg=what)
        assert not got[:, used:].any(), f"{what}: pad columns"
        rest = [i for i in range(N) if i not in {(top0 + i) % N for i in range(n)}]
        np.testing.assert_array_equal(got[rest].view(np.uint32), before[rest].view(np.uint32),
                                      err_msg=f"{what}: rows not written changed")


@pytest.mark.parametrize("Do,Da", rc.GATHER_SHAPES, ids=lambda v: str(v))
def test_gather_rows_bitwise_at_the_workgroup_edges(Do, Da):
    from oac_amd import ReplayBuffer
    rb = ReplayBuffer(rc.GATHER_ROWS, Space(Do), Space(Da), device=DEV)
    stride = rb.rows["row_stride"]
    rs = np.random.RandomState(5)
    bits = rs.randint(0, 1 << 32, (rc.GATHER_ROWS, stride), dtype=np.uint64).astype(np.uint32)
    rb.load_transitions(torch.from_numpy(bits.view(np.float32)).to(DEV))   # any bits, NaNs included
    for B in rc.GATHER_BATCHES:
        idx = rc.gather_indices(B)
        got = rb.gather(torch.from_numpy(idx).to(DEV))
        want = rb._storage[torch.from_numpy(idx).to(DEV).long()]
        torch.cuda.synchronize()
        assert got.shape == (B, stride)
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32),
                                      want.cpu().numpy().view(np.uint32), err_msg=f"B={B}")
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), bits[idx], err_msg=f"B={B}")
