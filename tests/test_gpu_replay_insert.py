"""ReplayBuffer._insert (oac_replay_insert) against oracle/replay_oracle.py's
one-by-one ring insert, through the branches no other test reaches: a path
that wraps, a path of exactly the capacity, paths longer than the capacity
from a nonzero _top (only the last N transitions stay, at the ring positions
sequential inserts would have left them), and longer than twice the capacity.

Fields are float64 values that float32 cannot represent, terminals uint8 (the
reference's host dtypes, replay_buffer.py:40-45): the stored row is the
float64 -> float32 rounding of each, bit for bit.  The row padding is zero in
every row (the insert kernel writes the whole row, padding as zero, and the
store starts zeroed); rows an insert does not reach keep their bits."""
import numpy as np
import pytest
import torch

from gpu_helpers import Space
from oracle.replay_oracle import CountReplayOracle

pytestmark = pytest.mark.gpu

N, Do, Da = 7, 3, 2
LENGTHS = [3, 6, 7, 10, 19, 1]   # _top before each: 0, 3, 2, 2, 5, 3


def _path(rs, n):
    # irrational multiples: none of these float64 values is a float32
    f = lambda *shape: rs.standard_normal(shape) * np.pi
    p = dict(observations=f(n, Do), actions=f(n, Da), rewards=f(n, 1),
             next_observations=f(n, Do), terminals=rs.randint(0, 2, (n, 1)).astype(np.uint8))
    for k in ("observations", "actions", "rewards", "next_observations"):
        assert not np.array_equal(p[k], p[k].astype(np.float32).astype(np.float64))
    return p


def _expected_rows(rb, orc):
    """The oracle's float64 ring as the float32 rows of the device store."""
    r = rb.rows
    want = np.zeros((N, r["row_stride"]), np.float32)
    want[:, r["off_obs"]:r["off_obs"] + Do] = np.float32(orc.obs)
    want[:, r["off_act"]:r["off_act"] + Da] = np.float32(orc.act)
    want[:, r["off_rew"]] = np.float32(orc.rew[:, 0])
    want[:, r["off_term"]] = orc.term[:, 0].astype(np.float32)
    want[:, r["off_next_obs"]:r["off_next_obs"] + Do] = np.float32(orc.next_obs)
    return want


@pytest.mark.parametrize("count", [False, True], ids=["plain", "count"])
def test_insert_sequence_equals_the_ring_oracle(count):
    from oac_amd import ReplayBuffer, ReplayBufferCount
    cls = ReplayBufferCount if count else ReplayBuffer
    rb = cls(N, Space(Do), Space(Da), device="cuda:0")
    orc = CountReplayOracle(N, Do, Da)
    r = rb.rows
    used = r["off_next_obs"] + Do
    assert used < r["row_stride"], "this shape has pad columns"
    rs = np.random.RandomState(0)
    seen_tops = []
    for step, n in enumerate(LENGTHS):
        path = _path(rs, n)
        top0 = rb._top
        seen_tops.append(top0)
        before = rb._storage.cpu().numpy().copy()
        written = sorted({(top0 + i) % N for i in range(n)})
        if count:   # nonzero counts everywhere: the insert zeroes exactly the rows it writes
            c0 = np.arange(1, N + 1, dtype=np.int32) + 10 * step
            rb._counts.copy_(torch.from_numpy(c0))
            orc.counts[:, 0] = c0
        rb.add_path(path)
        orc.add_path(path)
        torch.cuda.synchronize()
        got = rb._storage.cpu().numpy()
        what = f"insert {step} (n={n}, top {top0})"
        assert (rb._top, rb._size) == (orc.top, orc.size), what
        np.testing.assert_array_equal(got.view(np.uint32), _expected_rows(rb, orc).view(np.uint32),
                                      err_msg=what)
        assert not got[:, used:].any(), f"{what}: pad columns"
        rest = [i for i in range(N) if i not in written]
        np.testing.assert_array_equal(got[rest].view(np.uint32), before[rest].view(np.uint32),
                                      err_msg=f"{what}: rows not written changed")
        if count:
            cg = rb._counts.cpu().numpy()
            np.testing.assert_array_equal(cg, orc.counts[:, 0].astype(np.int32), err_msg=what)
            assert sorted(np.nonzero(cg == 0)[0].tolist()) == written, what
    # the sequence reached what it is for
    assert seen_tops == [0, 3, 2, 2, 5, 3]
    # snapshot -> a fresh buffer -> the same store
    ss = rb.get_snapshot()
    rb2 = cls(N, Space(Do), Space(Da), device="cuda:0")
    rb2.restore_from_snapshot(ss)
    assert torch.equal(rb2._storage, rb._storage)
    assert (rb2._top, rb2._size) == (rb._top, rb._size)
    if count:
        assert torch.equal(rb2._counts, rb._counts)


def test_add_sample_one_by_one_equals_add_path():
    """The same transitions through add_sample (n = 1 inserts, the rollout's
    call) leave the same store as the path inserts."""
    from oac_amd import ReplayBuffer
    a = ReplayBuffer(N, Space(Do), Space(Da), device="cuda:0")
    b = ReplayBuffer(N, Space(Do), Space(Da), device="cuda:0")
    rs = np.random.RandomState(0)
    for n in LENGTHS[:4]:
        path = _path(rs, n)
        a.add_path(path)
        for i in range(n):
            b.add_sample(path["observations"][i], path["actions"][i], path["rewards"][i],
                         path["next_observations"][i], path["terminals"][i])
    torch.cuda.synchronize()
    assert torch.equal(a._storage, b._storage)
    assert (a._top, a._size) == (b._top, b._size)
