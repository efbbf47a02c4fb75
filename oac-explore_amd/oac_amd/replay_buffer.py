"""Drop-in ``ReplayBuffer`` (/root/reference/replay_buffer.py:8-148) with the
transitions resident in HBM as fp32 rows.

Row layout (``trainer.row_layout``): ``[obs | act | rew | term | next_obs | pad]``.
Storing fp32 at insert time is bit-identical to the reference's float64 store
converted at sample time (``ptu.from_numpy(...).float()``, utils/core.py:45,
utils/pytorch_util.py:77): rounding f64->f32 is the same operation either way.

``random_batch(B)`` draws the indices exactly like the reference
(``np.random.randint(0, self._size, B)`` on numpy's global legacy MT19937,
replay_buffer.py:107) and returns a ``DeviceBatch``; ``SACTrainer.train``
gathers the rows on the GPU inside the step.  ``index_source='device'``
draws the same stream (np.random.seed(s) semantics) with the device MT19937
kernel instead, so no host work is needed per step.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .trainer import row_layout

BATCH_KEYS = ("observations", "actions", "rewards", "terminals", "next_observations")


def get_dim(space):
    """utils/env_utils.py:8-18."""
    if isinstance(space, (int, np.integer)):
        return int(space)
    if hasattr(space, "low"):
        return int(np.asarray(space.low).size)
    if hasattr(space, "n"):
        return int(space.n)
    if hasattr(space, "spaces"):
        return sum(get_dim(s) for s in space.spaces)
    if hasattr(space, "flat_dim"):
        return space.flat_dim
    raise TypeError(f"Unknown space: {space}")


class DeviceBatch(dict):
    """The batch dict ``random_batch`` returns: indices on the device plus a
    reference to the HBM store.  Reading a key (e.g. rl_algorithm's
    ``save_sampled_data`` path) gathers that field on the GPU on demand."""

    device_gather = True

    def __init__(self, buffer, indices=None, host_indices=None):
        super().__init__()
        self._buffer, self._indices = buffer, indices
        # host_indices: the np.random.randint draw itself (int64); the trainer
        # stages it through pinned memory inside its step (no pageable copy)
        self.host_indices = host_indices
        self.storage = buffer._storage
        self.batch_size = int(indices.numel() if indices is not None else len(host_indices))

    @property
    def indices(self):
        """The drawn indices as a device int32 tensor (uploaded on first use)."""
        if self._indices is None:
            self._indices = torch.from_numpy(self.host_indices.astype(np.int32)).to(
                self._buffer.device)
        return self._indices

    def __missing__(self, key):
        if key not in BATCH_KEYS:
            raise KeyError(key)
        rows = self._buffer.gather(self.indices)
        r = self._buffer.rows
        spans = dict(observations=(r["off_obs"], self._buffer.ob_dim),
                     actions=(r["off_act"], self._buffer.ac_dim),
                     rewards=(r["off_rew"], 1), terminals=(r["off_term"], 1),
                     next_observations=(r["off_next_obs"], self._buffer.ob_dim))
        o, n = spans[key]
        val = rows[:, o:o + n].contiguous()
        self[key] = val
        return val

    def keys(self):
        return list(BATCH_KEYS) + [k for k in dict.keys(self) if k not in BATCH_KEYS]


class ReplayBuffer(object):
    def __init__(self, max_replay_buffer_size, ob_space, action_space, device=None,
                 index_source="numpy", seed=None):
        self._ob_space, self._action_space = ob_space, action_space
        self.ob_dim, self.ac_dim = get_dim(ob_space), get_dim(action_space)
        self._max_replay_buffer_size = int(max_replay_buffer_size)
        self.rows = row_layout(self.ob_dim, self.ac_dim)
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        self._storage = torch.zeros(self._max_replay_buffer_size, self.rows["row_stride"],
                                    dtype=torch.float32, device=self.device)
        self._top = 0
        self._size = 0
        self.index_source = index_source
        self._mt = None
        if index_source == "device":
            self.seed_device_stream(0 if seed is None else seed)

    # ------------------------------------------------------------ insert
    def _rows_from(self, obs, act, rew, nobs, term):
        n = len(obs)
        r = self.rows
        out = np.zeros((n, r["row_stride"]), np.float32)
        out[:, r["off_obs"]:r["off_obs"] + self.ob_dim] = np.asarray(obs).reshape(n, -1)
        out[:, r["off_act"]:r["off_act"] + self.ac_dim] = np.asarray(act).reshape(n, -1)
        out[:, r["off_rew"]] = np.asarray(rew, np.float64).reshape(n)
        out[:, r["off_term"]] = np.asarray(term).reshape(n).astype(np.float32)
        out[:, r["off_next_obs"]:r["off_next_obs"] + self.ob_dim] = np.asarray(nobs).reshape(n, -1)
        return out

    def _write(self, rows_np):
        n = len(rows_np)
        t = torch.from_numpy(rows_np)
        done = 0
        while done < n:
            k = min(n - done, self._max_replay_buffer_size - self._top)
            self._storage[self._top:self._top + k].copy_(t[done:done + k])
            self._top = (self._top + k) % self._max_replay_buffer_size   # _advance, :101-104
            self._size = min(self._size + k, self._max_replay_buffer_size)
            done += k

    def _insert(self, obs, act, rew, nobs, term):
        """Ring insert of n transitions on the device (oac_replay_insert): the
        reference's host dtypes -- float64 fields, uint8 terminals
        (replay_buffer.py:40-45, 92-96) -- are copied once and packed into the
        fp32 rows by a HIP kernel (f64 -> f32 rounding identical to the
        reference's ptu.from_numpy(...).float() at sample time)."""
        n = len(obs)
        if n == 0:
            return
        N = self._max_replay_buffer_size
        top = self._top
        if n > N:   # sequential inserts of n > N rows leave the last N in place
            k = n - N
            top = (top + k) % N
            obs, act, rew, nobs, term = obs[k:], act[k:], rew[k:], nobs[k:], term[k:]
        m = len(obs)

        def dev(x, dt, shape):
            return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt).reshape(shape))).to(
                self.device)
        o = dev(obs, np.float64, (m, self.ob_dim))
        a = dev(act, np.float64, (m, self.ac_dim))
        r = dev(rew, np.float64, (m,))
        no = dev(nobs, np.float64, (m, self.ob_dim))
        t = dev(np.asarray(term).reshape(m).astype(np.uint8), np.uint8, (m,))
        lay = self.rows
        check(_lib.lib().oac_replay_insert(
            ptr(self._storage), lay["row_stride"], N, top, m, ptr(o), ptr(a), ptr(r), ptr(no),
            ptr(t), self.ob_dim, self.ac_dim, lay["off_obs"], lay["off_act"], lay["off_rew"],
            lay["off_term"], lay["off_next_obs"], stream_ptr()))
        self._on_insert(top, m)
        self._top = (self._top + n) % N                     # _advance, :101-104
        self._size = min(self._size + n, N)

    def _on_insert(self, top, m):
        """Hook: ring positions top .. top+m-1 (mod capacity) were just written."""

    def add_sample(self, observation, action, reward, next_observation, terminal,
                   env_info=None, **kwargs):
        """replay_buffer.py:88-99."""
        if hasattr(self._action_space, "n") and not hasattr(self._action_space, "low"):
            raise AssertionError("discrete action spaces are not supported")
        self._insert([observation], [action], [reward], [next_observation], [terminal])

    def add_path(self, path):
        """replay_buffer.py:50-82: one device insert per path."""
        if len(path["observations"]) == 0:
            return
        self._insert(path["observations"], path["actions"], path["rewards"],
                     path["next_observations"], path["terminals"])

    def add_paths(self, paths):
        for path in paths:
            self.add_path(path)

    def load_transitions(self, rows_fp32):
        """Bulk insert of pre-built device/host rows [n, row_stride] (synthetic fills)."""
        n = rows_fp32.shape[0]
        assert rows_fp32.shape[1] == self.rows["row_stride"] and n <= self._max_replay_buffer_size
        self._storage[:n].copy_(rows_fp32)
        self._top = n % self._max_replay_buffer_size
        self._size = n

    # ------------------------------------------------------------ sample
    def seed_device_stream(self, seed):
        st = np.zeros(625, np.uint32)
        check(_lib.lib().oac_mt_seed_host(ctypes.c_uint32(seed), st.ctypes.data_as(ctypes.c_void_p)))
        self._mt = torch.from_numpy(st.view(np.int32)).to(self.device)

    def sample_indices_device(self, count, out=None):
        """``count`` draws of np.random.randint(0, size) from the device stream."""
        if self._mt is None:
            raise RuntimeError("device index stream not seeded (index_source='device')")
        if out is None:
            out = torch.empty(count, dtype=torch.int32, device=self.device)
        check(_lib.lib().oac_replay_sample_indices(ptr(self._mt), ctypes.c_uint64(self._size),
                                                   int(count), ptr(out), stream_ptr()))
        return out

    def random_batch(self, batch_size):
        """replay_buffer.py:106-115."""
        if self.index_source == "device":
            return DeviceBatch(self, self.sample_indices_device(batch_size))
        return DeviceBatch(self, host_indices=np.random.randint(0, self._size, batch_size))

    def gather(self, indices):
        out = torch.empty(indices.numel(), self.rows["row_stride"], dtype=torch.float32,
                          device=self.device)
        check(_lib.lib().oac_replay_gather(ptr(self._storage), self.rows["row_stride"],
                                           ptr(indices), int(indices.numel()), ptr(out),
                                           stream_ptr()))
        return out

    # ------------------------------------------------------------ misc
    def get_dataset(self):
        r = self.rows
        return self._storage[:self._size, r["off_obs"]:r["off_obs"] + self.ob_dim]

    def num_steps_can_sample(self):
        return self._size

    def get_diagnostics(self):
        return OrderedDict([("size", self._size)])

    def end_epoch(self, epoch):
        return

    def get_snapshot(self):
        """Same keys and dtypes as replay_buffer.py:133-142."""
        r = self.rows
        s = self._storage.cpu().numpy().astype(np.float64)
        return dict(
            _observations=s[:, r["off_obs"]:r["off_obs"] + self.ob_dim],
            _next_obs=s[:, r["off_next_obs"]:r["off_next_obs"] + self.ob_dim],
            _actions=s[:, r["off_act"]:r["off_act"] + self.ac_dim],
            _rewards=s[:, r["off_rew"]:r["off_rew"] + 1],
            _terminals=s[:, r["off_term"]:r["off_term"] + 1].astype(np.uint8),
            _top=self._top, _size=self._size)

    def restore_from_snapshot(self, ss):
        for key in ss.keys():
            assert key in ("_observations", "_next_obs", "_actions", "_rewards", "_terminals",
                           "_top", "_size")
        rows = self._rows_from(ss["_observations"], ss["_actions"], ss["_rewards"],
                               ss["_next_obs"], ss["_terminals"])
        self._storage[:len(rows)].copy_(torch.from_numpy(rows))
        self._top, self._size = int(ss["_top"]), int(ss["_size"])


class ReplayBufferCount(ReplayBuffer):
    """ReplayBufferCount (replay_buffer.py:151-197): per-transition sample
    counts on the device.  random_batch's batch carries ``counts`` (the
    counts of the drawn rows BEFORE this draw, a device float32 [B, 1]; the
    reference returns a float64 copy) and every distinct drawn row's count is
    incremented once (numpy fancy-index ``+=``); ``priority_sample`` draws
    with p = 1/(count+1) (np.random.choice) -- the uniforms are numpy's own
    ``random_sample`` draws on the global stream, exactly the ones the
    reference's choice() consumes, the inverse-cdf search runs on the device
    (oac_replay_priority_sample)."""

    def __init__(self, max_replay_buffer_size, ob_space, action_space, priority_sample=False,
                 device=None, index_source="numpy", seed=None):
        super().__init__(max_replay_buffer_size, ob_space, action_space, device=device,
                         index_source=index_source, seed=seed)
        N = self._max_replay_buffer_size
        self._counts = torch.zeros(N, dtype=torch.int32, device=self.device)
        self._tags = torch.full((N,), -1, dtype=torch.int32, device=self.device)
        self._epoch = 0
        # dedupe epoch of the device ring path (train_from_ring with counts):
        # a device counter, disjoint from the host path's epochs 0, 1, 2, ...
        self._epoch_dev = torch.full((1,), 1 << 30, dtype=torch.int32, device=self.device)
        self.priority_sample = bool(priority_sample)
        self._scratch = None

    def _on_insert(self, top, m):
        """self._counts[self._top] = 0 for every inserted row (:177)."""
        N = self._max_replay_buffer_size
        first = min(m, N - top)
        self._counts[top:top + first].zero_()
        if m > first:
            self._counts[:m - first].zero_()

    def load_transitions(self, rows_fp32):
        super().load_transitions(rows_fp32)
        self._counts.zero_()

    def _priority_indices(self, B):
        L = _lib.lib()
        if self._scratch is None:
            n = int(L.oac_replay_priority_scratch_doubles(self._max_replay_buffer_size))
            self._scratch = torch.empty(n, dtype=torch.float64, device=self.device)
        u = torch.from_numpy(np.random.random_sample(B)).to(self.device)   # choice()'s draws
        idx = torch.empty(B, dtype=torch.int32, device=self.device)
        check(L.oac_replay_priority_sample(ptr(self._counts), self._size, ptr(u), int(B),
                                           ptr(self._scratch), ptr(idx), stream_ptr()))
        return idx

    def random_batch(self, batch_size):
        """replay_buffer.py:180-197."""
        B = int(batch_size)
        if self.priority_sample:
            idx = self._priority_indices(B)
        else:
            idx = super().random_batch(B).indices
        counts = torch.empty(B, dtype=torch.float32, device=self.device)
        check(_lib.lib().oac_replay_counts_update(ptr(self._counts), ptr(self._tags), ptr(idx), B,
                                                  self._epoch, ptr(counts), stream_ptr()))
        self._epoch += 1
        batch = DeviceBatch(self, idx)
        batch["counts"] = counts.view(B, 1)
        return batch

    def device_count_state(self):
        """(counts, tags, epoch) device tensors for trainer.train_from_ring:
        the ring path's steps read / bump these counts like random_batch
        (uniform draws only: priority sampling draws from numpy's stream)."""
        if self.priority_sample:
            raise NotImplementedError("priority_sample draws on the host (np.random.choice); "
                                      "train with random_batch batches")
        return (self._counts, self._tags, self._epoch_dev)

    def get_snapshot(self):
        ss = super().get_snapshot()
        ss["_counts"] = self._counts.cpu().numpy().astype(np.float64).reshape(-1, 1)
        return ss

    def restore_from_snapshot(self, ss):
        ss = dict(ss)
        counts = ss.pop("_counts", None)
        super().restore_from_snapshot(ss)
        if counts is not None:
            self._counts.copy_(torch.from_numpy(np.asarray(counts).reshape(-1).astype(np.int32)))


class DeviceIndexStream:
    """A ring of pre-drawn batch indices for ``SACTrainer.train_from_ring``:
    2*chunk step slots, refilled one chunk ahead by the device MT19937 kernel
    (sequential in the stream, so the index sequence equals
    ``np.random.seed(seed); randint(0, size, B)`` called once per step).

    A ring step reads slot ``batch_counter % slots`` (gather_kernel), so stream
    step k lives in slot ``(start + k) % slots``: ``start`` is the trainer's
    batch counter (``step_state[1]``) at the stream's first step -- 0 for a
    fresh trainer, the number of gradient steps already taken otherwise.  With
    another ``start`` than the trainer's counter the steps read slots in a
    rotated order (the first draws skipped, or a stale half first)."""

    def __init__(self, buffer, batch_size, chunk=64, seed=1, start=0):
        self.buf, self.B, self.chunk = buffer, int(batch_size), int(chunk)
        self.slots = 2 * self.chunk
        self.start = int(start)
        if self.start < 0:
            raise ValueError("start is a batch counter: it must be >= 0")
        self.ring = torch.empty(self.slots * self.B, dtype=torch.int32, device=buffer.device)
        buffer.seed_device_stream(seed)
        self.t = 0
        self._fill(0)
        self._fill(self.chunk)

    def _fill(self, k0):
        """Stream steps k0 .. k0 + chunk - 1 into their slots (two pieces when
        they wrap the ring's end; the stream carries from call to call)."""
        s0 = (self.start + k0) % self.slots
        first = min(self.chunk, self.slots - s0)
        self.buf.sample_indices_device(first * self.B,
                                       out=self.ring[s0 * self.B:(s0 + first) * self.B])
        if first < self.chunk:
            self.buf.sample_indices_device((self.chunk - first) * self.B,
                                           out=self.ring[:(self.chunk - first) * self.B])

    def before_step(self, n_steps=1):
        """Call before each ring step (or block of n_steps consecutive steps,
        n_steps dividing the chunk): refill the half that was just consumed."""
        if self.chunk % n_steps or self.t % n_steps:
            raise ValueError("n_steps must divide the ring chunk and the step count")
        if self.t > 0 and self.t % self.chunk == 0:
            self._fill(self.t + self.chunk)   # over the slots of steps t - chunk .. t - 1
        self.t += n_steps


class ReplayBufferNoResampling(ReplayBuffer):
    """Drop-in ``ReplayBufferNoResampling`` (replay_buffer_no_resampling.py:8-173),
    the buffer of ``--no_resampling``: every transition is drawn exactly once and
    its slot is then handed to the next insert.

    The rows, the ordered list of live slots (``_valid_indeces``) and the ring of
    freed slots (``indices_to_replace``) live on the device; the host keeps the
    reference's five counters (``_top``, ``_bottom_indexes``, ``_top_indexes``,
    ``_size`` and the list's length) with the reference's own arithmetic, the
    ring's aliasing included (N freed slots make the ring read as empty).

    ``random_batch(B)`` takes B distinct POSITIONS of the list:
    ``index_source='numpy'`` draws ``np.random.choice(len, size=B,
    replace=False)`` on the global stream -- the reference's
    ``np.random.choice(self._valid_indeces, ...)`` picks the list's entries at
    exactly these positions and leaves the stream in the same state;
    ``'device'`` draws them with Floyd's sampling on Philox (no host work
    proportional to the list, no copy back, no synchronisation).  The take
    kernels gather the slots in draw order, push them on the ring and compact
    the list (oac_replay_nr_take, two launches).

    Deviations from the reference:

    1. An insert of m rows with live + m > capacity raises ``RuntimeError``
       before changing anything (the reference wraps ``_top`` onto a live slot,
       overwrites it and lists it twice).  The ``--no_resampling`` schedule never
       gets there.
    2. ``restore_from_snapshot`` restores every key of ``get_snapshot`` (the
       reference asserts on a misspelt attribute and cannot run).
    3. ``random_batch(B)`` with B > live raises numpy's ``ValueError`` with
       numpy's words from either index source; nothing changes.

    A take handles at most 4096 positions (they are sorted in LDS).
    ``get_dataset`` raises: the reference class has none, and the live rows are
    scattered over the store."""

    MAX_BATCH = 4096
    SNAPSHOT_KEYS = ("_observations", "_next_obs", "_actions", "_rewards", "_terminals", "_top",
                     "_indices_to_replace", "_bottom_indexes", "_top_indexes", "_valid_indeces",
                     "_size")

    def __init__(self, max_replay_buffer_size, ob_space, action_space, device=None,
                 index_source="numpy", seed=None):
        if index_source not in ("numpy", "device"):
            raise ValueError(f"ReplayBufferNoResampling: index_source {index_source!r}")
        super().__init__(max_replay_buffer_size, ob_space, action_space, device=device,
                         index_source="numpy")
        N = self._max_replay_buffer_size
        if N >= 1 << 31:
            raise ValueError(f"ReplayBufferNoResampling: capacity {N} >= 2^31")
        self.index_source = index_source
        self._valid = [torch.zeros(N, dtype=torch.int32, device=self.device) for _ in range(2)]
        self._cur = 0        # which list buffer is current
        self._live = 0       # len(_valid_indeces)
        self._queue = torch.zeros(N, dtype=torch.int32, device=self.device)
        self._bottom_indexes = 0
        self._top_indexes = 0
        self._shift = torch.empty(self.MAX_BATCH, dtype=torch.int32, device=self.device)
        self._seed, self._draws = 0, 0
        self.seed_device_stream(0 if seed is None else seed)

    # ------------------------------------------------------------ insert
    def _insert(self, obs, act, rew, nobs, term):
        """add_sample (:98-122) for m rows in one launch: the first q rows go to
        the ring's slots, the rest to _top onward; every slot is appended to
        the live list."""
        m = len(obs)
        if m == 0:
            return
        N = self._max_replay_buffer_size
        if self._live + m > N:
            raise RuntimeError(
                f"ReplayBufferNoResampling: inserting {m} rows over {self._live} live rows "
                f"exceeds the capacity {N} (a live row would be written over)")
        q = (self._top_indexes - self._bottom_indexes) % N

        def dev(x, dt, shape):
            return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt).reshape(shape))).to(
                self.device)
        o = dev(obs, np.float64, (m, self.ob_dim))
        a = dev(act, np.float64, (m, self.ac_dim))
        r = dev(rew, np.float64, (m,))
        no = dev(nobs, np.float64, (m, self.ob_dim))
        t = dev(np.asarray(term).reshape(m).astype(np.uint8), np.uint8, (m,))
        lay = self.rows
        check(_lib.lib().oac_replay_nr_insert(
            ptr(self._storage), lay["row_stride"], N, self._top, ptr(self._queue),
            self._bottom_indexes, q, ptr(self._valid[self._cur]), self._live, m, ptr(o), ptr(a),
            ptr(r), ptr(no), ptr(t), self.ob_dim, self.ac_dim, lay["off_obs"], lay["off_act"],
            lay["off_rew"], lay["off_term"], lay["off_next_obs"], stream_ptr()))
        k = min(m, q)                                   # _advance, :116-122
        self._bottom_indexes = (self._bottom_indexes + k) % N
        self._top = (self._top + m - k) % N
        self._size = min(self._size + m, N)
        self._live += m

    def load_transitions(self, rows_fp32):
        """Bulk fill of an EMPTY buffer with pre-built rows [n, row_stride]: slots
        0 .. n-1 in order, as n add_sample calls would leave them."""
        if self._live or self._top or self._top_indexes != self._bottom_indexes:
            raise RuntimeError("ReplayBufferNoResampling.load_transitions: the buffer is not empty")
        n = rows_fp32.shape[0]
        assert rows_fp32.shape[1] == self.rows["row_stride"] and n <= self._max_replay_buffer_size
        self._storage[:n].copy_(rows_fp32)
        self._valid[self._cur][:n].copy_(torch.arange(n, dtype=torch.int32, device=self.device))
        self._top = n % self._max_replay_buffer_size
        self._size = self._live = n

    # ------------------------------------------------------------ sample
    def seed_device_stream(self, seed):
        """Key of the device position draw; restarts its draw counter."""
        self._seed, self._draws = int(seed) & (2 ** 64 - 1), 0

    def sample_positions_device(self, n, batch_size, draw_counter=None):
        """The device draw alone: B distinct positions of [0, n) for draw
        ``draw_counter`` (default: the buffer's counter, which is NOT advanced)."""
        B = int(batch_size)
        d = self._draws if draw_counter is None else int(draw_counter)
        out = torch.empty(max(B, 1), dtype=torch.int32, device=self.device)
        check(_lib.lib().oac_replay_nr_sample_positions(
            int(n), B, ctypes.c_uint64(self._seed), ctypes.c_uint64(d), ptr(out), stream_ptr()))
        return out[:B]

    def _check_batch(self, B):
        if B > self._live:   # numpy's own refusal, np.random.choice(live, B, replace=False)
            raise ValueError("Cannot take a larger sample than population when 'replace=False'")
        if B < 1:
            raise ValueError("ReplayBufferNoResampling: batch_size must be >= 1")
        if B > self.MAX_BATCH:
            raise ValueError(f"ReplayBufferNoResampling: batch_size {B} > {self.MAX_BATCH}")

    def _take_device(self, positions, B):
        """One take (positions: device int32 [B], or None = device draw):
        (slots, positions used) as device tensors; the counters advance as
        add_indices_to_replace (:91-96) moves them."""
        N = self._max_replay_buffer_size
        idx = torch.empty(B, dtype=torch.int32, device=self.device)
        pos = torch.empty(B, dtype=torch.int32, device=self.device)
        src, dst = self._valid[self._cur], self._valid[1 - self._cur]
        check(_lib.lib().oac_replay_nr_take(
            ptr(src), self._live, ptr(positions), B, ptr(self._queue), N, self._top_indexes,
            ptr(idx), ptr(pos), ptr(dst), ptr(self._shift), ctypes.c_uint64(self._seed),
            ctypes.c_uint64(self._draws), stream_ptr()))
        self._cur = 1 - self._cur
        self._live -= B
        self._top_indexes = (self._top_indexes + B) % N
        self._size -= B
        return idx, pos

    def _take(self, positions):
        """Take the list's entries at the given distinct host positions (any
        order): the drawn slots in that order, a device int32 tensor."""
        p = np.asarray(positions).reshape(-1)
        B = len(p)
        self._check_batch(B)
        p = p.astype(np.int64)
        if p.min() < 0 or p.max() >= self._live or len(np.unique(p)) != B:
            raise ValueError("ReplayBufferNoResampling._take: positions must be distinct and in "
                             f"[0, {self._live})")
        return self._take_device(torch.from_numpy(p.astype(np.int32)).to(self.device), B)[0]

    def random_batch(self, batch_size):
        """replay_buffer_no_resampling.py:124-141."""
        B = int(batch_size)
        self._check_batch(B)   # before the stream moves
        if self.index_source == "device":
            idx, _ = self._take_device(None, B)
            self._draws += 1
        else:
            idx = self._take(np.random.choice(self._live, size=B, replace=False))
        return DeviceBatch(self, idx)

    def add_indices_to_replace(self, indices):
        """:91-96 for slot VALUES: each is pushed on the ring and its first
        occurrence leaves the list.  Not on random_batch's path: it downloads
        the list to find the positions (a synchronisation)."""
        indices = [int(i) for i in indices]
        if not indices:
            return
        lst = self._valid[self._cur][:self._live].cpu().numpy()
        order = np.argsort(lst, kind="stable")
        at = np.searchsorted(lst[order], indices)
        if (at >= len(lst)).any() or (lst[order][np.minimum(at, len(lst) - 1)] != indices).any() \
                or len(set(indices)) != len(indices):
            raise ValueError("list.remove(x): x not in list")
        self._take(order[at])

    # ------------------------------------------------------------ misc
    def get_dataset(self):
        raise NotImplementedError(
            "ReplayBufferNoResampling has no get_dataset (the reference class has none; the live "
            "rows are scattered over the store)")

    def sample_indices_device(self, count, out=None):
        raise NotImplementedError(
            "ReplayBufferNoResampling draws without replacement: use random_batch")

    def valid_indices(self):
        """The live list (_valid_indeces) as a device int32 tensor, in order."""
        return self._valid[self._cur][:self._live]

    def get_snapshot(self):
        """The reference's eleven keys and dtypes (:154-167)."""
        ss = super().get_snapshot()
        ss.update(
            _indices_to_replace=self._queue.cpu().numpy().astype(np.uint64),
            _bottom_indexes=self._bottom_indexes, _top_indexes=self._top_indexes,
            _valid_indeces=[int(i) for i in self.valid_indices().cpu().numpy()])
        return ss

    def restore_from_snapshot(self, ss):
        """Every key of get_snapshot (the reference's evident intent, :169-173)."""
        for key in ss.keys():
            assert key in self.SNAPSHOT_KEYS, key
        N = self._max_replay_buffer_size
        lst = np.asarray(ss["_valid_indeces"], np.int64).reshape(-1)
        q = np.asarray(ss["_indices_to_replace"]).reshape(-1)
        if len(lst) > N or len(q) != N:
            raise ValueError("ReplayBufferNoResampling.restore_from_snapshot: wrong capacity")
        if (len(lst) and (lst.min() < 0 or lst.max() >= N)) or q.max() >= N:
            raise ValueError("ReplayBufferNoResampling.restore_from_snapshot: a slot >= capacity")
        rows = self._rows_from(ss["_observations"], ss["_actions"], ss["_rewards"],
                               ss["_next_obs"], ss["_terminals"])
        self._storage[:len(rows)].copy_(torch.from_numpy(rows))
        self._queue.copy_(torch.from_numpy(q.astype(np.int64).astype(np.int32)))
        self._valid[self._cur][:len(lst)].copy_(torch.from_numpy(lst.astype(np.int32)))
        self._live = len(lst)
        self._top, self._size = int(ss["_top"]), int(ss["_size"])
        self._bottom_indexes = int(ss["_bottom_indexes"])
        self._top_indexes = int(ss["_top_indexes"])
