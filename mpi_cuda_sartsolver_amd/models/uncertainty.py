"""Monte-Carlo error bars: noisy replicas of a frame as columns of the multi-frame engine, per-voxel mean and spread.

``perturbed_frames`` runs the noise kernel (csrc/kernels/noise.hip): replica r >= 1 of a pixel is
``max(g + sigma z, 0)`` with ``sigma^2 = abs^2 + shot g + (rel g)^2`` and ``z`` the Philox4x32-10 normal of (seed,
frame time, global pixel, replica) -- ``utils.philox`` restates it in NumPy. ``replica_moments`` runs the moments kernel
(csrc/kernels/moments64.hip): mean and unbiased standard deviation per voxel over the replicas that count, in index
order and two passes. ``solve_replicas`` puts them together on a ``MultiFrameSARTSolver``: the nominal frame and its
replicas are cold columns of one batch, so N replicas cost about one batched sweep per iteration.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from ..ops import hip
from ..utils.philox import time_bits
from .sart import SolveResult

CHUNK = 64  # replicas per launch of the noise kernel


def _device(device) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def perturbed_frames(g, time: float, nrep: int, abs: float = 0.0, shot: float = 0.0, rel: float = 0.0,  # noqa: A002
                     seed: int = 0, pixel0: int = 0, device=None) -> np.ndarray:
    """``[nrep + 1, n]``: row 0 is ``g``, row r its replica r, generated on the GPU in chunks of 64 replicas.
    ``g[p]`` is global pixel ``pixel0 + p`` (a rank's slice gives the bits of the whole frame's call)."""
    gh = np.ascontiguousarray(np.asarray(g, dtype=np.float64).reshape(-1))
    if nrep < 0:
        raise ValueError("nrep must be >= 0")
    n = gh.size
    out = np.empty((nrep + 1, n), dtype=np.float64)
    out[0] = gh
    if nrep == 0 or n == 0:
        return out
    dev = _device(device)
    k = hip()
    ldo = (n + 63) // 64 * 64
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        gd = torch.from_numpy(gh).to(dev)
        buf = torch.empty((min(CHUNK, nrep), ldo), dtype=torch.float64, device=dev)
        for r0 in range(1, nrep + 1, CHUNK):
            m = min(CHUNK, nrep + 1 - r0)
            k.noise_replicas(gd.data_ptr(), n, int(pixel0), time_bits(time), r0, m, float(abs), float(shot),
                             float(rel), int(seed) & 0xFFFFFFFFFFFFFFFF, buf.data_ptr(), ldo, stream)
            out[r0: r0 + m] = buf[:m, :n].cpu().numpy()
    return out


def replica_moments(X, use=None, device=None):
    """``(mean, std, count)`` per voxel over the rows of ``X`` ``[n, nvoxel]`` with ``use[r]`` set (None: all):
    ``count`` rows counted; std is NaN for count < 2, mean NaN for count 0."""
    Xh = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if Xh.ndim != 2:
        raise ValueError("X must be [n, nvoxel]")
    n, nvoxel = Xh.shape
    u = np.ones(n, dtype=np.uint8) if use is None else np.ascontiguousarray(np.asarray(use).ravel() != 0, dtype=np.uint8)
    if u.size != n:
        raise ValueError("use must have one entry per row of X")
    dev = _device(device)
    k = hip()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        Xd = torch.from_numpy(Xh).to(dev)
        ud = torch.from_numpy(u).to(dev)
        mean = torch.empty(nvoxel, dtype=torch.float64, device=dev)
        std = torch.empty(nvoxel, dtype=torch.float64, device=dev)
        k.moments64(Xd.data_ptr(), nvoxel, nvoxel, n, ud.data_ptr(), mean.data_ptr(), std.data_ptr(), stream)
        return mean.cpu().numpy(), std.cpu().numpy(), int(u.sum())


@dataclass
class ReplicaResult:
    nominal: SolveResult          # the unperturbed frame's solve (column 0)
    replicas: List[SolveResult]   # [nrep]
    frames: np.ndarray            # [nrep + 1, npixel] what was solved
    mean: np.ndarray              # [nvoxel] over the replicas that count
    std: np.ndarray               # [nvoxel] unbiased
    count: int                    # replicas that did not stop on a non-finite iterate


def solve_replicas(solver, g, time: float, nrep: int, abs: float = 0.0, shot: float = 0.0,  # noqa: A002
                   rel: float = 0.0, seed: int = 0, pixel0: Optional[int] = None) -> ReplicaResult:
    """The frame ``g`` (this rank's pixels) and ``nrep`` noisy replicas of it as cold columns of one ``solve_batch`` on
    a ``MultiFrameSARTSolver`` (one rank), then the moments of the replicas' solutions."""
    if solver.comm.world_size != 1:
        raise NotImplementedError("solve_replicas runs on one rank (the native driver's --replicas takes several)")
    if nrep < 2:
        raise ValueError("nrep must be >= 2")
    if min(abs, shot, rel) < 0 or max(abs, shot, rel) <= 0:
        raise ValueError("the noise terms must be >= 0 and one of them > 0")
    frames = perturbed_frames(g, time, nrep, abs, shot, rel, seed, pixel0 or 0, device=solver.dev)
    cols = solver.solve_batch(frames)
    use = np.array([not r.nonfinite for r in cols[1:]], dtype=np.uint8)
    mean, std, count = replica_moments(np.stack([r.solution for r in cols[1:]]), use, device=solver.dev)
    return ReplicaResult(cols[0], cols[1:], frames, mean, std, count)
