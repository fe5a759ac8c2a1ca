"""NumPy restatement of the noise definition of ``--replicas`` (csrc/kernels/philox.hpp; README "Replicas").

Philox4x32-10 with key = (seed low word, seed high word) and counter = (global pixel index, replica, low and high word
of the frame time's IEEE-754 bits), one standard normal per counter by Box-Muller's cosine branch from 53 + 53 bits, and
the perturbation ``g' = max(g + sigma z, 0)`` with ``sigma^2 = abs^2 + shot g + (rel g)^2`` of the pixels with
``g >= 0`` (a negative pixel is the solver's exclusion marker and stays). Everything in fp64; the tests hold the host
binding and the device kernel against these functions.
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    """counter: [..., 4] and key: [..., 2] 32-bit words (broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) & _MASK for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) & _MASK for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def time_bits(time: float) -> int:
    """The IEEE-754 bit pattern of the frame time (0.0 and -0.0 differ)."""
    return int(np.array(time, dtype=np.float64).view(np.uint64))


def noise_words(seed: int, time: float, pixels, replica: int) -> np.ndarray:
    """The four output words of every pixel's counter: [n, 4] uint32."""
    pixels = np.asarray(pixels, dtype=np.uint64).reshape(-1)
    bits, seed = time_bits(time), int(seed) & 0xFFFFFFFFFFFFFFFF
    counter = np.empty((pixels.size, 4), dtype=np.uint64)
    counter[:, 0] = pixels & _MASK
    counter[:, 1] = int(replica) & 0xFFFFFFFF
    counter[:, 2] = bits & 0xFFFFFFFF
    counter[:, 3] = bits >> 32
    return philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))


def noise_normals(seed: int, time: float, pixels, replica: int) -> np.ndarray:
    """One standard normal per global pixel index of `pixels`, for this seed, frame time and replica."""
    w = noise_words(seed, time, pixels, replica).astype(np.uint64)
    a = (w[:, 0] << np.uint64(21)) + (w[:, 1] >> np.uint64(11))
    b = (w[:, 2] << np.uint64(21)) + (w[:, 3] >> np.uint64(11))
    u1 = (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53  # (0, 1]; a + 1 <= 2^53 is exact in fp64
    u2 = b.astype(np.float64) * 2.0 ** -53                   # [0, 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def noise_sigma(g, abs: float, shot: float, rel: float) -> np.ndarray:  # noqa: A002  (the issue's names)
    g = np.asarray(g, dtype=np.float64)
    rg = rel * g
    with np.errstate(invalid="ignore"):  # excluded pixels (g < 0) are not used
        return np.sqrt(abs * abs + shot * g + rg * rg)


def perturb(g, time: float, nrep: int, abs: float, shot: float, rel: float, seed: int,  # noqa: A002
            pixel0: int = 0) -> np.ndarray:
    """[nrep + 1, n]: row 0 is g, row r >= 1 its replica r; g[p] is global pixel pixel0 + p."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    out = np.empty((nrep + 1, g.size), dtype=np.float64)
    out[0] = g
    pixels = np.arange(g.size, dtype=np.uint64) + np.uint64(pixel0)
    sigma = noise_sigma(g, abs, shot, rel)
    for r in range(1, nrep + 1):
        z = noise_normals(seed, time, pixels, r)
        with np.errstate(invalid="ignore"):
            out[r] = np.where(g < 0, g, np.maximum(g + sigma * z, 0.0))
    return out
