"""CPU restatement of the device noise generator -- TEST INFRASTRUCTURE ONLY
(the checker for tests/ and nothing else; the product path never imports it).

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
as 1, 2, 3", SC'11) and the Box-Muller draw built on it by
oac-explore_amd/csrc/kernels.h (philox4x32_10, philox_normal).  Written from
the published algorithm and that header; the reference project has no Philox.

Element ``idx`` of draw ``stream`` at step ``counter`` of a generator seeded
``seed``:

    counter words  {idx >> 1, stream, counter lo, counter hi}
    key            {seed lo, seed hi}
    u1, u2 = (float32(word >> 8) + 0.5f) * 2^-24   of output words 0 and 1
    r = sqrt(-2 log u1),  th = float32(2 pi) * u2
    value = r cos th (idx even) | r sin th (idx odd)

so the two elements of a pair 2k, 2k+1 share one Philox block.  The uniforms
are formed in float32 exactly as the kernel forms them (the + 0.5f rounds once
word >> 8 reaches 2^23); ``dtype`` selects the precision of the transcendental
part only.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter4, key2):
    """Ten rounds of Philox4x32 on ``counter4`` (four 32-bit words, scalars or
    equally shaped arrays) under ``key2`` (two 32-bit words).  uint64 arrays
    masked to 32 bits; returns the four output words."""
    c = [np.asarray(x, np.uint64) & _MASK for x in counter4]
    k0, k1 = (np.asarray(k, np.uint64) & _MASK for k in key2)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]          # 32 x 32 -> 64 bits: no overflow
        hi0, lo0 = p0 >> _S32, p0 & _MASK
        hi1, lo1 = p1 >> _S32, p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def _uniform24(word):
    f32 = np.float32
    return ((word >> np.uint64(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)


def philox_normal(seed, counter, stream, idx, dtype=np.float64):
    """kernels.h philox_normal for every element of ``idx`` (any shape).
    dtype=np.float32: every operation in float32, as the kernel; np.float64:
    log / sqrt / sin / cos in double on the same float32 u1, u2 and the same
    float32 2 pi."""
    seed, counter = int(seed), int(counter)
    idx = np.asarray(idx, np.uint64)
    z = np.zeros(idx.shape, np.uint64)
    c = philox4x32_10([idx >> np.uint64(1), z + np.uint64(stream),
                       z + np.uint64(counter & 0xFFFFFFFF), z + np.uint64((counter >> 32) & 0xFFFFFFFF)],
                      [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    u1, u2 = _uniform24(c[0]), _uniform24(c[1])
    two_pi = np.float32(6.283185307179586)
    if np.dtype(dtype) == np.float32:
        r = np.sqrt(np.float32(-2.0) * np.log(u1))
        th = two_pi * u2
    else:
        u1, u2 = u1.astype(np.float64), u2.astype(np.float64)
        r = np.sqrt(-2.0 * np.log(u1))
        th = np.float64(two_pi) * u2
    odd = (idx & np.uint64(1)).astype(bool)
    return np.where(odd, r * np.sin(th), r * np.cos(th)).astype(dtype)
