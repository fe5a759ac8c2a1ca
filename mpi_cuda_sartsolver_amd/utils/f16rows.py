"""Row-scaled f16 storage of a ray-transfer matrix: the NumPy definition of the format.

Every row p of the shard is stored as ``H[p, v] = rne_f16(A[p, v] * s_p)`` with a power-of-two scale ``s_p`` of its
own, chosen from the row's largest finite magnitude ``m_p = mant * 2^e`` (``mant`` in [0.5, 1)) as
``s_p = 2^clamp(14 - e, -120, 120)``: scaled row maxima lie in [2^13, 2^14), the convention of the multi-frame
engine's f16 operand pieces (``mf_f16_shift``, csrc/kernels/multiframe_glue.hip). All-zero rows get ``s_p = 1``.
The conversion is IEEE round-to-nearest-even and keeps f16 subnormals; a NaN is stored as the canonical quiet NaN
0x7e00, +-inf stays +-inf. The matrix the solvers solve is ``H / s_p``, exact in fp32.

Entries below 2^-27 of their row's maximum fall into f16's subnormal range (they lose precision), entries below
2^-38 of it (half of the smallest subnormal 2^-24, over a scaled maximum of at least 2^13) are stored as zero.

This module is the oracle of the device conversion kernel (``launch_f32_to_f16_rows``, csrc/kernels/projection.hip),
which reproduces it bit for bit.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

SHIFT_MAX = 120          # |scale exponent| bound: the scale and its inverse stay normal fp32
F16_MIN_NORMAL = 2.0 ** -14


class F16Rows(NamedTuple):
    bits: np.ndarray         # uint16 [n, nvoxel]: f16 bit patterns of A * s_p
    scales: np.ndarray       # fp32 [n]: s_p
    dequantised: np.ndarray  # fp32 [n, nvoxel]: H / s_p
    flushed: int             # non-zero finite inputs stored as zero or as an f16 subnormal


def row_scale_exponents(A: np.ndarray) -> np.ndarray:
    """The exponent of s_p per row (int32)."""
    A = np.asarray(A, dtype=np.float32)
    mag = np.where(np.isfinite(A), np.abs(A), np.float32(0))
    m = mag.max(axis=1) if A.shape[1] else np.zeros(A.shape[0], dtype=np.float32)
    _, e = np.frexp(m)  # m = mant 2^e, mant in [0.5, 1); 0 -> (0, 0)
    return np.where(m > 0, np.clip(14 - e, -SHIFT_MAX, SHIFT_MAX), 0).astype(np.int32)


def quantise_rows_f16(A) -> F16Rows:
    """Quantise a dense fp32 block of whole rows. Returns (bits, scales, dequantised, flushed)."""
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float32))
    if A.ndim != 2:
        raise ValueError("quantise_rows_f16 takes a 2-d block of whole rows")
    s = row_scale_exponents(A)
    scale = np.ldexp(np.float32(1), s).astype(np.float32)
    inv = np.ldexp(np.float32(1), -s).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        scaled = (A * scale[:, None]).astype(np.float32)
        h = scaled.astype(np.float16)
    bits = h.view(np.uint16).copy()
    bits[np.isnan(A)] = 0x7E00
    h = bits.view(np.float16)
    with np.errstate(invalid="ignore", under="ignore"):
        deq = (h.astype(np.float32) * inv[:, None]).astype(np.float32)
        small = np.isfinite(A) & (A != 0) & (np.abs(h.astype(np.float32)) < np.float32(F16_MIN_NORMAL))
    return F16Rows(bits, scale, deq, int(np.count_nonzero(small)))


def dequantise_rows_f16(bits, scales) -> np.ndarray:
    """fp32 H / s_p from stored bits and scales."""
    h = np.ascontiguousarray(np.asarray(bits, dtype=np.uint16)).view(np.float16).astype(np.float32)
    inv = (np.float32(1) / np.asarray(scales, dtype=np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore", under="ignore"):
        return (h * inv[:, None]).astype(np.float32)
