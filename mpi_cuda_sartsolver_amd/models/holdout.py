"""Hold-out cross-validation: a frame solved as measured and with each of K folds of its pixels excluded, the fp64
projections of the solutions scored on the pixels they did not see.

``holdout_sums`` runs the scoring kernel (csrc/kernels/holdout64.hip): per column and camera the sums of ``(g - f)^2`` and
``g^2`` and the count over the held-out pixels and over the others, fp64 without contraction in a fixed order -- a value
depends on its column, its camera and the inputs alone. ``holdout_scores`` is the native score rule
(csrc/native/holdout.cpp; ``utils/holdout.py`` restates it in NumPy). ``solve_holdout`` puts them together on a
``MultiFrameSARTSolver``: the masked frames are cold columns of one batch (a pixel with ``g < 0`` is the solver's
exclusion marker), with a ladder of Laplacian weights if asked, so a whole cross-validation costs about one batched sweep
per iteration.

Voxels seen only by held-out pixels are constrained by the cold start and the Laplacian alone, and the ray densities
still count the held-out rows (as they do for saturated pixels).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..ops import hip, native
from ..utils.holdout import SUM_NAMES, masked_frames
from .fit import fit_forward_device, group_size
from .sart import SolveResult
from .uncertainty import _device


def holdout_sums(F, g, ell, threshold: float, fold, held, camera_pixels: Sequence[int], device=None) -> np.ndarray:
    """``[n, ncam, 6]`` (``utils.holdout.SUM_NAMES``' order) for the fitted images ``F`` ``[n, ldf >= npixel]`` (NumPy,
    or a contiguous fp64 device tensor) of ``n`` columns of the frame ``g`` ``[npixel]``: ``ell`` the ray lengths,
    ``fold`` the fold per pixel, ``held`` ``[n]`` the fold each column held out (-1: none), ``camera_pixels`` the pixels
    per camera in order (their sum is ``npixel``)."""
    cams = np.asarray(camera_pixels, dtype=np.int64).reshape(-1)
    if cams.size < 1 or np.any(cams < 0):
        raise ValueError("camera_pixels must hold at least one camera of >= 0 pixels")
    npixel = int(cams.sum())
    gh = np.ascontiguousarray(np.asarray(g, dtype=np.float64).reshape(-1))
    eh = np.ascontiguousarray(np.asarray(ell, dtype=np.float64).reshape(-1))
    fh = np.ascontiguousarray(np.asarray(fold, dtype=np.int32).reshape(-1))
    hh = np.ascontiguousarray(np.asarray(held, dtype=np.int32).reshape(-1))
    if gh.size != npixel or eh.size != npixel or fh.size != npixel:
        raise ValueError(f"g, ell and fold must be [{npixel}]: the cameras' pixels")
    if isinstance(F, torch.Tensor):
        if F.dtype != torch.float64 or F.dim() != 2 or not F.is_contiguous() or not F.is_cuda:
            raise ValueError("a device F must be a contiguous float64 [n, ldf] tensor")
        dev, Fd = F.device, F
    else:
        dev = _device(device)
        Fd = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(F, dtype=np.float64)))).to(dev)
    n, ldf = int(Fd.shape[0]), int(Fd.shape[1])
    if ldf < npixel or npixel < 1:
        raise ValueError("F rows must hold the cameras' pixels (at least one)")
    if hh.size != n or not 1 <= n <= 65535:
        raise ValueError("held must hold one entry per row of F (1 .. 65535 rows)")
    starts = np.concatenate([[0], np.cumsum(cams)]).astype(np.int64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        gd, ed, fd, hd, sd = (torch.from_numpy(a).to(dev) for a in (gh, eh, fh, hh, starts))
        sums = torch.empty((n, cams.size, len(SUM_NAMES)), dtype=torch.float64, device=dev)
        hip().holdout64(Fd.data_ptr(), ldf, n, gd.data_ptr(), ed.data_ptr(), float(threshold), fd.data_ptr(),
                        hd.data_ptr(), sd.data_ptr(), int(cams.size), sums.data_ptr(), stream)
        return sums.cpu().numpy()


@dataclass
class HoldoutScores:
    cv_error: np.ndarray         # [nb] RMS prediction error over the held-out pixels (each valid pixel once)
    cv_relative: np.ndarray      # [nb] the same against the RMS of the measurement
    train_error: np.ndarray      # [nb] RMS residual of the unmasked column over the pixels it was fitted to
    cv_error_camera: np.ndarray  # [nb, ncam]
    eligible: np.ndarray         # [nb] uint8
    selected: int
    found: bool


def holdout_scores(sums, ok=None, fallback: int = 0) -> HoldoutScores:
    """The native scores of one composite frame: ``sums`` ``[nb, K + 1, ncam, 6]``, ``ok`` ``[nb, K + 1]`` (default: all
    columns count), ``fallback`` the ladder entry taken when none is eligible."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    okv = (np.ones(s.shape[:2], dtype=np.uint8) if ok is None
           else np.ascontiguousarray(np.asarray(ok) != 0, dtype=np.uint8))
    cv, rel, train, cam, elig, sel, found = native().holdout_scores(s, okv, int(fallback))
    return HoldoutScores(np.asarray(cv), np.asarray(rel), np.asarray(train), np.asarray(cam), np.asarray(elig),
                         int(sel), bool(found))


@dataclass
class HoldoutResult:
    betas: np.ndarray                 # [nb] the ladder (one entry, the solver's weight, without one)
    folds: np.ndarray                 # [npixel] int32
    frames: np.ndarray                # [K + 1, npixel] what was solved per weight (row 0: the frame)
    columns: List[List[SolveResult]]  # [nb][K + 1]
    sums: np.ndarray                  # [nb, K + 1, ncam, 6]
    scores: HoldoutScores
    result: SolveResult               # the selected weight's unmasked column


def solve_holdout(solver, g, folds, K: int, betas=None, camera_pixels: Optional[Sequence[int]] = None) -> HoldoutResult:
    """The frame ``g`` ``[npixel]`` and its ``K`` masked copies (``folds``: int32 per pixel, values 0 .. K - 1) at every
    weight of ``betas`` (increasing; None: the solver's own weight) as ``nb (K + 1)`` cold columns of ``solve_batch`` on
    a ``MultiFrameSARTSolver`` (one rank; built with ``frame_betas=True`` when a ladder is given). The solutions are
    projected through the matrix as stored by the fit kernels and scored on the device (``holdout64``); the native
    scores select the weight (fallback: the entry nearest to the solver's weight)."""
    if solver.comm.world_size != 1:
        raise NotImplementedError("solve_holdout runs on one rank (the native driver's --holdout takes several)")
    rtm = solver.rtm
    gh = np.asarray(g, dtype=np.float64).reshape(-1)
    fh = np.asarray(folds, dtype=np.int32).reshape(-1)
    if gh.size != rtm.npixel or fh.size != rtm.npixel:
        raise ValueError(f"g and folds must be [{rtm.npixel}]")
    if K < 1 or fh.min() < 0 or fh.max() >= K:
        raise ValueError("folds must lie within 0 .. K - 1")
    cams = [rtm.npixel] if camera_pixels is None else [int(c) for c in camera_pixels]
    if sum(cams) != rtm.npixel:
        raise ValueError("camera_pixels must add up to the frame's pixels")
    if betas is None:
        b = np.array([solver.params.beta_laplace], dtype=np.float64)
    else:
        b = np.asarray(betas, dtype=np.float64).ravel()
        if b.size < 1 or not np.all(np.isfinite(b)) or b[0] < 0 or not np.all(np.diff(b) > 0):
            raise ValueError("betas must be increasing values >= 0")
        if not solver.frame_betas:
            raise ValueError("a ladder needs a solver built with frame_betas=True")
    nb, nc = b.size, K + 1
    frames = masked_frames(gh, fh, K)
    cols = solver.solve_batch(np.tile(frames, (nb, 1)), betas=None if betas is None else np.repeat(b, nc))
    dev = rtm.device
    sparse = getattr(rtm, "nnz", None) is not None
    ldx, ldf = int(rtm.ld), int(rtm.nrows_pad)
    held = np.tile(np.arange(-1, K, dtype=np.int32), nb)
    thr = float(solver.params.ray_length_threshold)
    sums = np.empty((nb * nc, len(cams), len(SUM_NAMES)), dtype=np.float64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        group = group_size(rtm)
        Xd = torch.zeros((group, ldx), dtype=torch.float64, device=dev)
        Fd = torch.zeros((group, ldf), dtype=torch.float64, device=dev)
        Xt = torch.zeros((ldx, 8), dtype=torch.float64, device=dev) if sparse else None
        Xd[0, : rtm.nvoxel] = 1.0
        fit_forward_device(rtm, Xd, 1, Fd, Xt=Xt, stream=stream)
        ell = Fd[0, : rtm.npixel].cpu().numpy()
        for j0 in range(0, nb * nc, group):
            n = min(group, nb * nc - j0)
            X = np.stack([cols[j].solution for j in range(j0, j0 + n)])
            Xd[:n, : rtm.nvoxel].copy_(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)))
            fit_forward_device(rtm, Xd, n, Fd, Xt=Xt, stream=stream)
            sums[j0: j0 + n] = holdout_sums(Fd[:n], gh, ell, thr, fh, held[j0: j0 + n], cams)
    sums = sums.reshape(nb, nc, len(cams), len(SUM_NAMES))
    ok = np.array([not c.nonfinite for c in cols], dtype=np.uint8).reshape(nb, nc)
    fallback = int(native().holdout_fallback(b, float(solver.params.beta_laplace)))
    sc = holdout_scores(sums, ok, fallback)
    columns = [cols[i * nc: (i + 1) * nc] for i in range(nb)]
    return HoldoutResult(b, fh, frames, columns, sums, sc, columns[sc.selected][0])
