"""oracle/philox_oracle.py, the CPU restatement the GPU noise tests compare
the device draws with (tests/test_gpu_noise.py): Philox4x32-10 known answers,
and the construction of csrc/kernels.h philox_normal -- counter words
{idx >> 1, stream, counter}, key = seed, Box-Muller on two 24-bit uniforms --
giving independent standard normals across elements, streams and steps.

Everything here is deterministic (fixed seeds and counters): the statistical
bounds are 4 sigma of each estimator under N(0, 1) at N samples (the KS bound
the alpha = 0.001 critical value 1.95 / sqrt(N)), properties of the design,
not a flaky draw."""
import numpy as np
import pytest
from scipy import stats

from oracle.philox_oracle import philox4x32_10, philox_normal

N = 69632   # = 4096 * 17, the largest eps draw of tests/test_gpu_noise.py (> 256 * 256)
CASES = [(0, 0), (0, 1), (3, 17), (12345678901234, 2 ** 33)]

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = tuple(int(x) for x in philox4x32_10(ctr, key))
    assert got == want, [hex(x) for x in got]


def test_known_answers_vectorised():
    """The array form (what philox_normal uses) equals the scalar form."""
    ctr = [np.array([k[0][i] for k in KAT], np.uint64) for i in range(4)]
    # one key per call: the three vectors have three keys
    for j, (_, key, want) in enumerate(KAT):
        got = philox4x32_10(ctr, key)
        assert tuple(int(w[j]) for w in got) == want


@pytest.fixture(scope="module")
def draws():
    idx = np.arange(N)
    return {(s, c, st): philox_normal(s, c, st, idx, np.float64)
            for s, c in CASES for st in (1, 2)}


def _corr(a, b):
    return abs(float(np.corrcoef(a, b)[0, 1]))


@pytest.mark.parametrize("seed,counter", CASES)
@pytest.mark.parametrize("stream", [1, 2])
def test_draws_are_standard_normal(draws, seed, counter, stream):
    x = draws[(seed, counter, stream)]
    assert x.dtype == np.float64 and x.shape == (N,) and np.isfinite(x).all()
    got = dict(mean=abs(x.mean()), std=abs(x.std() - 1.0),
               ks=stats.kstest(x, "norm").statistic,
               skew=abs(stats.skew(x)), kurt=abs(stats.kurtosis(x)),
               lag1=_corr(x[:-1], x[1:]), amax=np.abs(x).max())
    bound = dict(mean=4 / np.sqrt(N), std=4 / np.sqrt(2 * N), ks=1.95 / np.sqrt(N),
                 skew=4 * np.sqrt(6 / N), kurt=4 * np.sqrt(24 / N), lag1=4 / np.sqrt(N),
                 # u1 >= 2^-25: r <= sqrt(-2 ln 2^-25) = 5.887
                 amax=np.sqrt(-2 * np.log(2.0 ** -25)))
    bad = {k: (float(got[k]), float(bound[k])) for k in got if not got[k] <= bound[k]}
    assert not bad, (bad, got)


@pytest.mark.parametrize("seed,counter", CASES)
def test_streams_are_uncorrelated(draws, seed, counter):
    a, b = draws[(seed, counter, 1)], draws[(seed, counter, 2)]
    assert not np.array_equal(a, b)
    assert _corr(a, b) <= 4 / np.sqrt(N)


def test_consecutive_counters_are_uncorrelated():
    idx = np.arange(N)
    a = philox_normal(3, 5, 1, idx, np.float64)
    b = philox_normal(3, 6, 1, idx, np.float64)
    assert _corr(a, b) <= 4 / np.sqrt(N)


def test_high_words_of_seed_and_counter_are_used():
    """The key's and the counter's high words reach the block: a seed or
    counter differing only above bit 32 draws different values."""
    idx = np.arange(64)
    base = philox_normal(5, 7, 1, idx)
    assert not np.array_equal(base, philox_normal(5 + 2 ** 32, 7, 1, idx))
    assert not np.array_equal(base, philox_normal(5, 7 + 2 ** 32, 1, idx))


def test_pairs_share_one_block():
    """Elements 2k and 2k+1 are the cos / sin halves of block k (counter word
    0 = idx >> 1): x^2 + y^2 = -2 ln u1 of that block, formed here from
    philox4x32_10 directly.  A draw per element index (idx in place of
    idx >> 1) gives equally normal values and fails this."""
    seed, counter, stream, n = 3, 17, 1, 4096
    x = philox_normal(seed, counter, stream, np.arange(2 * n), np.float64)
    k = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, np.uint64)
    c = philox4x32_10([k, z + np.uint64(stream), z + np.uint64(counter), z], [seed, 0])
    u1 = ((c[0] >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    r2 = -2.0 * np.log(u1.astype(np.float64))
    np.testing.assert_allclose(x[0::2] ** 2 + x[1::2] ** 2, r2, rtol=1e-12, atol=0)


def test_float32_form_is_close_to_float64():
    """The all-float32 form (the kernel's arithmetic) stays within a few 1e-7
    of the double form: this distance is the unit of the GPU tests' allowance."""
    idx = np.arange(N)
    for s, c in CASES:
        a = philox_normal(s, c, 1, idx, np.float32)
        assert a.dtype == np.float32
        d = np.abs(a.astype(np.float64) - philox_normal(s, c, 1, idx, np.float64)).max()
        assert 0 < d < 4e-6, d   # |x| < 6: ulp(4) = 4.8e-7, a handful of roundings
