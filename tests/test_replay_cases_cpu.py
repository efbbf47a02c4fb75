"""The input conditions of tests/replay_cases.py, asserted for every row (no
GPU; nothing is excluded): the exactness of the dyadic priority rows, the
margin of the general ones, that the table reaches every edge it names, and the
host-only side of the replay ABI (the size checks that precede any launch)."""
import ctypes

import numpy as np
import pytest

import replay_cases as rc

DYADIC_IDS = [c.name for c in rc.DYADIC]
GENERAL_IDS = [c.name for c in rc.GENERAL]


def test_table_reaches_the_edges_it_names():
    sizes = [c.size for c in rc.DYADIC]
    assert sizes[:9] == [1, 2, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 1, 4_194_304]
    assert rc.SCAN_BLOCK == 4096 and rc.MAX_SIZE == 4_194_304 == max(sizes)
    assert rc.SCAN_BLOCK - 1 in sizes and rc.SCAN_BLOCK + 1 in sizes      # each side of a block
    assert any(s > 2 * rc.SCAN_BLOCK for s in sizes)                      # more than two blocks
    assert any(c.size < c.capacity for c in rc.DYADIC)
    assert rc.dyadic_class_sizes(4097) == (4095, 2, 0, 0)
    assert rc.dyadic_class_sizes(rc.MAX_SIZE) == (1 << 20, 1 << 20, 1 << 21, 0)
    # the tie on a block boundary: u = cdf[4095] exactly, expecting index 4096
    reached = 0
    for c in rc.DYADIC:
        if c.size < rc.SCAN_BLOCK + 1:
            continue
        counts, u, idx, tie = rc.dyadic_reference(c)
        at = {j: (a, b) for j, a, b in tie}
        a, b = at[rc.SCAN_BLOCK - 1]
        assert u[a] == rc.oracle_cdf(counts[:c.size])[rc.SCAN_BLOCK - 1]
        assert idx[a] == rc.SCAN_BLOCK and idx[b] == rc.SCAN_BLOCK - 1
        reached += 1
    assert reached >= 6
    assert [(c.size, c.B) for c in rc.GENERAL] == [(4095, 1000), (4097, 1000), (8193, 2048),
                                                   (200003, 4096)]
    assert rc.COUNT_BATCHES == (1, 255, 256, 257, 1025, 4096) and rc.COUNT_ROWS == 50
    assert rc.MT_COUNTS == (0, 1, 623, 624, 625, 0, 1247, 1, 1249, 624)
    assert rc.MT_SEQUENCE_SIZES == (1000, 2 ** 20 + 1)
    assert rc.MT_SINGLE_SIZES == (2 ** 32, 2 ** 31 + 1, 2 ** 16, 2 ** 16 - 1, 2 ** 16 + 1)
    assert rc.GATHER_BATCHES == (1, 15, 16, 17, 250)


@pytest.mark.parametrize("name", DYADIC_IDS)
def test_dyadic_rows_are_exact(name):
    c = rc.DYADIC_BY_NAME[name]
    counts, u, idx, tie = rc.dyadic_reference(c)
    n = c.size
    assert counts.shape == (c.capacity,) and set(np.unique(counts[:n])) <= set(rc.DYADIC_COUNTS)
    assert tuple(int((counts[:n] == k).sum()) for k in rc.DYADIC_COUNTS) == rc.dyadic_class_sizes(n)
    w = 1.0 / (counts[:n].astype(np.float64) + 1.0)
    # every partial sum in integer arithmetic (units of 1/8): numpy's sequential
    # float64 cumsum equals it, so no partial sum was rounded
    w8 = (8 // (counts[:n].astype(np.int64) + 1))
    assert np.array_equal(w8 / 8.0, w)
    exact = np.cumsum(w8)
    total8 = int(exact[-1])
    assert total8 % 8 == 0 and (total8 // 8) & (total8 // 8 - 1) == 0, "total is a power of two"
    assert total8 < 2 ** 53
    seq = np.cumsum(w)
    assert np.array_equal(seq * 8.0, exact.astype(np.float64))
    # another association: the weights permuted, summed pairwise (np.sum) block
    # by block as the device's two-level scan groups them, and unpermuted again
    perm = np.random.RandomState(c.seed + 7).permutation(n)
    assert np.sum(w[perm]) * 8.0 == total8
    starts = np.arange(0, n, rc.SCAN_BLOCK)
    blocks = np.add.reduceat(w, starts)
    pre = np.concatenate([[0.0], np.cumsum(blocks)[:-1]])
    two_level = np.concatenate([pre[b] + np.cumsum(w[s:s + rc.SCAN_BLOCK])
                                for b, s in enumerate(starts)])
    assert np.array_equal(two_level, seq)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    assert np.array_equal(np.cumsum(w[perm][inv]), seq)
    # the oracle's normalisation is exact and ends at 1
    cdf = rc.oracle_cdf(counts[:n])
    assert cdf[-1] == 1.0
    assert np.array_equal(cdf * (total8 / 8.0), seq)
    assert (np.diff(cdf) > 0).all()
    # the uniforms: in [0, 1), u * total exact (a power-of-two scaling), ties representable
    assert u[0] == 0.0 and u[1] == 1.0 - 2.0 ** -53 and np.nextafter(u[1], 2.0) == 1.0
    assert (u >= 0).all() and (u < 1).all() and len(u) == 2 + 2 * len(tie) + rc.N_RANDOM_U
    assert [j for j, _, _ in tie] == rc.tie_rows(n)
    t = u * (total8 / 8.0)
    assert np.array_equal(t / (total8 / 8.0), u)
    for j, a, b in tie:
        assert u[a] == cdf[j] and u[a] * (total8 / 8.0) == seq[j]          # exactly on the step
        assert u[b] < u[a] and np.nextafter(u[b], 1.0) == u[a]
        assert idx[a] == j + 1 and idx[b] == j                             # side='right'
    # the reference itself: index = #{j : W_j <= u * total} on the exact sums
    assert np.array_equal(idx, np.searchsorted(seq, t, side="right"))
    assert idx[0] == 0 and idx[1] == n - 1
    assert idx.min() >= 0 and idx.max() <= n - 1
    if n > 2 * rc.SCAN_BLOCK:
        assert len(set(idx // rc.SCAN_BLOCK)) >= 3, "draws in at least three scan blocks"


@pytest.mark.parametrize("name", GENERAL_IDS)
def test_general_rows_keep_the_margin(name):
    """Every draw of the row at least MARGIN x (the float64 cdf's largest
    distance from the long double cdf) away from the nearest cdf step; the
    seed is part of the row, no draw is left out.  Measured: 1.16e7 (4095),
    4.19e4 (4097), 1.04e7 (8193), 5.69e3 (200003)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "long double is wider than float64 here"
    c = rc.GENERAL_BY_NAME[name]
    counts, u, idx = rc.general_reference(c)
    assert counts.shape == (c.size,) and counts.min() == 0 and counts.max() == 39
    assert u.shape == (c.B,) and idx.shape == (c.B,)
    np.random.seed(c.seed + 1)
    assert np.array_equal(np.random.random_sample(c.B), u)
    ratio, noise = rc.general_margin_ratio(c)
    print(f"{name}: margin ratio {ratio:.3g} (cdf rounding {noise:.3g})")
    assert noise > 0 and ratio >= rc.MARGIN, (name, ratio)
    full = c.size // rc.SCAN_BLOCK
    assert set(range(full)) <= set((idx // rc.SCAN_BLOCK).tolist()), "every full scan block drawn from"


def test_counts_reference_counts_a_repeated_index_once():
    c = np.zeros(5, np.int64)
    before = rc.bump(c, np.array([1, 1, 3, 1]))
    assert before.tolist() == [0, 0, 0, 0] and c.tolist() == [0, 1, 0, 1, 0]
    before = rc.bump(c, np.array([3, 4, 3]))
    assert before.tolist() == [1, 0, 1] and c.tolist() == [0, 1, 0, 2, 1]


def test_mt_rows_straddle_the_624_word_block():
    """At size 1000 about 2.4% of the words are rejected, so the call counts
    end below, on and above a 624-word block; at 2^20 + 1 about half are."""
    assert sum(rc.MT_COUNTS) > 8 * 624   # at least eight twists in the sequence
    for size in rc.MT_SEQUENCE_SIZES:
        calls = rc.randint_calls(5, size, rc.MT_COUNTS)
        assert [len(x) for x in calls] == list(rc.MT_COUNTS)
        whole = np.random.RandomState(5).randint(0, size, sum(rc.MT_COUNTS))
        assert np.array_equal(np.concatenate(calls), whole)   # the state carries between calls
    big = np.random.RandomState(5).randint(0, 2 ** 32, 2000)
    assert big.max() >= 2 ** 31 and big.dtype == np.int64


def test_gather_indices_hold_the_edges():
    for B in rc.GATHER_BATCHES:
        idx = rc.gather_indices(B)
        assert idx.shape == (B,) and idx.min() >= 0 and idx.max() == rc.GATHER_ROWS - 1
        if B > 1:
            assert 0 in idx and len(set(idx.tolist())) < B


def test_insert_shapes_have_the_strides_named():
    from oac_amd.trainer import row_layout
    strides = [row_layout(*s)["row_stride"] for s in rc.INSERT_SHAPES]
    assert strides == [12, 12, 772]
    for (Do, Da), st in zip(rc.INSERT_SHAPES[:2], strides):
        assert row_layout(Do, Da)["off_next_obs"] + Do == st      # no pad column
    assert strides[2] > 256                                        # wider than one insert block
    assert [row_layout(*s)["row_stride"] // 4 for s in rc.GATHER_SHAPES] == [2, 193]


# ------------------------------------------------------------- host-only ABI
def test_priority_sample_size_bounds_precede_any_launch():
    """size 0 and 4,194,305 are refused by name with null buffers (nothing is
    launched or read); B = 0 returns 0."""
    from oac_amd import _lib as L
    lib = L.lib()
    for size in (0, rc.MAX_SIZE + 1, -1):
        assert lib.oac_replay_priority_sample(None, size, None, 4, None, None, None) != 0
        msg = lib.oac_last_error()
        assert b"priority sample" in msg and b"[1, 4194304]" in msg, msg
    assert lib.oac_replay_priority_sample(None, rc.MAX_SIZE, None, 0, None, None, None) == 0
    assert lib.oac_replay_priority_scratch_doubles(rc.MAX_SIZE) >= rc.MAX_SIZE + 1024
    assert lib.oac_replay_priority_scratch_doubles(4097) >= 4097 + 2


def test_sample_indices_size_bounds_precede_any_launch():
    from oac_amd import _lib as L
    lib = L.lib()
    for size in (0, 2 ** 32 + 1):
        assert lib.oac_replay_sample_indices(None, ctypes.c_uint64(size), 4, None, None) != 0
        assert b"[1, 2^32]" in lib.oac_last_error()
