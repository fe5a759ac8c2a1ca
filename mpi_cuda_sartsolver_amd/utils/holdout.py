"""NumPy restatement of the hold-out definitions of ``--holdout`` (csrc/native/holdout.cpp, csrc/kernels/holdout64.hip;
README "Hold-out"), bit for bit.

Folds: pixel mode takes ``w = philox4x32_10((global pixel, 0, 0x484F4C44, 0); key = (seed low word, seed high word))``
and ``fold(p) = (uint64(w[0]) K) >> 32`` -- a function of (seed, global pixel) alone; camera mode gives a pixel the index
of its camera in composite order. Column ``c >= 1`` of a frame has ``g_p = -1`` (the solver's exclusion marker) where
``fold(p) = c - 1`` and ``g_p >= 0``. ``sums_reference`` follows the scoring kernel's order of additions: 256 lanes, each
over its pixels ``start + t, + 256, ...`` in order, then the tree ``s[t] += s[t + stride]`` for stride 128 .. 1.
``scores`` restates the native scores of one composite frame.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .philox import philox4x32_10

COUNTER_TAG = 0x484F4C44  # "HOLD"
SUM_NAMES = ("held_residual2", "held_measured2", "held_pixels", "kept_residual2", "kept_measured2", "kept_pixels")
LANES = 256


def folds(n: int, K: int = 0, seed: int = 0, pixel0: int = 0, camera_pixels: Optional[Sequence[int]] = None) -> np.ndarray:
    """int32 ``[n]``: the folds of the global pixels ``pixel0 .. pixel0 + n - 1``. ``camera_pixels`` (pixels per camera
    in composite order) selects camera mode; else ``K`` (2 .. 32) pixel folds keyed by ``seed``."""
    if camera_pixels is not None:
        ends = np.cumsum(np.asarray(camera_pixels, dtype=np.int64))
        p = np.arange(n, dtype=np.int64) + int(pixel0)
        if n and (ends.size == 0 or p[-1] >= ends[-1]):
            raise ValueError("pixels beyond the cameras' pixels")
        return np.searchsorted(ends, p, side="right").astype(np.int32)
    if not 2 <= K <= 32:
        raise ValueError("K must be within 2 .. 32")
    if pixel0 + n > 1 << 32:
        raise ValueError("pixel folds apply to fewer than 2^32 pixels")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    counter = np.zeros((n, 4), dtype=np.uint64)
    counter[:, 0] = np.arange(n, dtype=np.uint64) + np.uint64(pixel0)
    counter[:, 2] = COUNTER_TAG
    w = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    return ((w[:, 0].astype(np.uint64) * np.uint64(K)) >> np.uint64(32)).astype(np.int32)


def masked_frames(g, fold, K: int) -> np.ndarray:
    """``[K + 1, n]``: row 0 is ``g``, row c >= 1 has -1 where ``fold == c - 1`` and ``g >= 0``."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    fold = np.asarray(fold).reshape(-1)
    if fold.size != g.size:
        raise ValueError("g and fold must have one entry per pixel")
    out = np.repeat(g[None, :], K + 1, axis=0)
    with np.errstate(invalid="ignore"):
        valid = g >= 0
    for c in range(1, K + 1):
        out[c, valid & (fold == c - 1)] = -1.0
    return out


def _lane_tree(terms: np.ndarray) -> float:
    """The kernel's sum of ``terms`` (a camera's pixels in order; 0 where a pixel does not count: adding +0 to a value
    that is >= 0 or NaN changes nothing)."""
    n = terms.size
    rows = -(-n // LANES) if n else 0
    padded = np.zeros(max(rows, 1) * LANES, dtype=np.float64)
    padded[:n] = terms
    acc = np.zeros(LANES, dtype=np.float64)
    for row in padded.reshape(-1, LANES):
        acc = acc + row
    stride = LANES // 2
    while stride > 0:
        acc[:stride] = acc[:stride] + acc[stride: 2 * stride]
        stride //= 2
    return float(acc[0])


def sums_reference(F, g, ell, threshold: float, fold, held, camera_pixels: Sequence[int]) -> np.ndarray:
    """``[n, ncam, 6]`` (``SUM_NAMES``' order) in the scoring kernel's order of operations: ``F`` ``[n, >= npixel]``
    fitted images, ``g``, ``ell`` and ``fold`` ``[npixel]``, ``held`` ``[n]`` (-1: nothing held out)."""
    F = np.atleast_2d(np.asarray(F, dtype=np.float64))
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    ell = np.asarray(ell, dtype=np.float64).reshape(-1)
    fold = np.asarray(fold).reshape(-1)
    held = np.asarray(held).reshape(-1)
    starts = np.concatenate([[0], np.cumsum(np.asarray(camera_pixels, dtype=np.int64))])
    npixel = int(starts[-1])
    if g.size < npixel or ell.size < npixel or fold.size < npixel or F.shape[1] < npixel or held.size != F.shape[0]:
        raise ValueError("operands do not cover the cameras' pixels")
    with np.errstate(invalid="ignore"):
        valid = (g[:npixel] >= 0) & (ell[:npixel] > threshold)
    gg = g[:npixel] * g[:npixel]
    out = np.zeros((F.shape[0], len(camera_pixels), len(SUM_NAMES)), dtype=np.float64)
    for j in range(F.shape[0]):
        with np.errstate(invalid="ignore", over="ignore"):
            d = g[:npixel] - F[j, :npixel]
            dd = d * d
        hold = valid & (fold[:npixel] == held[j]) if held[j] >= 0 else np.zeros(npixel, dtype=bool)
        keep = valid & ~hold
        for m in range(len(camera_pixels)):
            sl = slice(int(starts[m]), int(starts[m + 1]))
            for q, (mask, term) in enumerate(((hold, dd), (hold, gg), (hold, None), (keep, dd), (keep, gg), (keep, None))):
                t = np.ones(npixel) if term is None else term
                out[j, m, q] = _lane_tree(np.where(mask[sl], t[sl], 0.0))
    return out


def fallback_index(betas, beta: float) -> int:
    """The ladder entry nearest to ``beta`` (ties to the smaller index)."""
    b = np.asarray(betas, dtype=np.float64).reshape(-1)
    return int(np.argmin(np.abs(b - beta)))


def _rms(num, den):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(den == 0.0, np.nan, np.sqrt(np.divide(num, den)))


def scores(sums, ok, fallback: int = 0) -> Dict[str, np.ndarray]:
    """The scores of one composite frame from ``sums`` ``[nb, K + 1, ncam, 6]`` and ``ok`` ``[nb, K + 1]`` (the column
    did not stop on a non-finite iterate): ``cv_error``, ``cv_relative``, ``train_error`` ``[nb]``, ``cv_error_camera``
    ``[nb, ncam]``, ``eligible`` ``[nb]``, ``selected``, ``found``. Sums run over the columns 1 .. K outer and the
    cameras inner, in index order."""
    s = np.asarray(sums, dtype=np.float64)
    okv = np.asarray(ok) != 0
    nb, nc, ncam, _ = s.shape
    num, norm, count = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    cnum, ccount = np.zeros((nb, ncam)), np.zeros((nb, ncam))
    for c in range(1, nc):
        for m in range(ncam):
            num = num + s[:, c, m, 0]
            norm = norm + s[:, c, m, 1]
            count = count + s[:, c, m, 2]
        cnum = cnum + s[:, c, :, 0]
        ccount = ccount + s[:, c, :, 2]
    tnum, tcount = np.zeros(nb), np.zeros(nb)
    for m in range(ncam):
        tnum = tnum + s[:, 0, m, 3]
        tcount = tcount + s[:, 0, m, 5]
    cv = _rms(num, count)
    eligible = okv.all(axis=1) & np.isfinite(cv)
    selected, found = int(fallback), 0
    for i in range(nb):
        if eligible[i] and (not found or cv[i] < cv[selected]):
            selected, found = i, 1
    return {"cv_error": cv, "cv_relative": _rms(num, norm), "train_error": _rms(tnum, tcount),
            "cv_error_camera": _rms(cnum, ccount), "eligible": eligible.astype(np.uint8),
            "selected": np.int32(selected), "found": np.uint8(found)}
