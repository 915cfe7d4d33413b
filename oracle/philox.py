"""Plain numpy restatement of the library's normal-draw stream (model_kernels.hpp: philox_round / randn_body).

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011) followed by the Box-Muller transform.
Pair i of the stream (seed, stream) is generated from counter (i lo, i hi, stream lo, stream hi) under key (seed lo, seed hi):
the four output words give a = c1:c0 and b = c3:c2, u = ((x >> 11) + 0.5) * 2^-53 for x in (a, b), and

    z[2 i] = sqrt(-2 log u1) cos(2 pi u2),   z[2 i + 1] = sqrt(-2 log u1) sin(2 pi u2)

with the sine value of the last pair dropped when the count is odd.  The uniforms are formed in float64 exactly as the device
forms them (the + 0.5 rounds for x >> 11 >= 2^52, and near u = 1 that rounding moves sqrt(-2 log u) by far more than an ulp);
the logarithm and the trigonometric functions run in np.longdouble, so the reference is at least as accurate as the device.

This pins the stream layout: a change of the generator, the counter / key assignment or the transform must update this file.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key bumps (golden ratio, sqrt(3) - 1)
ROUNDS = 10
_MASK32 = np.uint64(0xFFFFFFFF)
# 2 pi to more digits than a long double holds (np.longdouble(np.pi) would only carry the float64 value)
_TWO_PI = np.longdouble("6.283185307179586476925286766559005768394")


def philox4x32_10(ctr, key):
    """ctr: (..., 4), key: (..., 2) integer arrays of 32-bit words (broadcast against each other).
    Returns the (..., 4) uint32 output block."""
    ctr = np.asarray(ctr, dtype=np.uint64) & _MASK32
    key = np.asarray(key, dtype=np.uint64) & _MASK32
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., j], shape).copy() for j in range(4)]
    k0 = np.broadcast_to(key[..., 0], shape).copy()
    k1 = np.broadcast_to(key[..., 1], shape).copy()
    with np.errstate(over="ignore"):
        for _ in range(ROUNDS):
            p0 = np.uint64(M0) * c[0]                 # 32 x 32 -> 64 bits: exact in uint64
            p1 = np.uint64(M1) * c[2]
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK32,
                 (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK32]
            k0 = (k0 + np.uint64(W0)) & _MASK32
            k1 = (k1 + np.uint64(W1)) & _MASK32
    return np.stack(c, axis=-1).astype(np.uint32)


def _split64(v):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError(f"{v} is not a 64-bit unsigned value")
    return v & 0xFFFFFFFF, v >> 32


def _uniform(lo, hi):
    """((hi:lo >> 11) + 0.5) * 2^-53, rounded in float64 as the device rounds it."""
    x = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def randn_reference(seed, stream, count):
    """The first `count` values of the library's N(0, 1) stream (seed, stream), as float64."""
    count = int(count)
    if count < 0:
        raise ValueError("count must be non-negative")
    if count == 0:
        return np.zeros(0)
    s_lo, s_hi = _split64(seed)
    t_lo, t_hi = _split64(stream)
    i = np.arange((count + 1) // 2, dtype=np.uint64)
    ctr = np.stack([i & _MASK32, i >> np.uint64(32), np.full_like(i, t_lo), np.full_like(i, t_hi)], axis=-1)
    c = philox4x32_10(ctr, np.array([s_lo, s_hi], dtype=np.uint64))
    u1 = _uniform(c[:, 0], c[:, 1]).astype(np.longdouble)
    u2 = _uniform(c[:, 2], c[:, 3]).astype(np.longdouble)
    rad = np.sqrt(-2 * np.log(u1))
    ang = _TWO_PI * u2
    z = np.empty(2 * len(i), dtype=np.longdouble)
    z[0::2] = rad * np.cos(ang)
    z[1::2] = rad * np.sin(ang)
    return z[:count].astype(np.float64)
