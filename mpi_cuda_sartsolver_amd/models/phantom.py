"""Phantom studies: reconstruct known emissivities and score what comes back.

``phantom_sums(X, t)`` runs the scoring kernel (csrc/kernels/phantom64.hip): ten fp64 values per column of ``X`` against
the truth ``t`` -- ``s_t, s_x, s_tt, s_xx, s_xt, s_dd`` (sums of t, x, t^2, x^2, x t, (x - t)^2), ``s_in`` (the sum of x
over the voxels with t > 0) and ``m_d, m_t, m_x`` (the maxima of \\|x - t\\|, t, x). ``phantom_scores(sums)`` restates the
native scores (csrc/native/phantom.cpp) in NumPy, bit for bit: each is one correctly rounded division (the cosine: a
product, a square root and a division), a zero denominator gives NaN. ``solve_phantoms`` puts them together on a
``MultiFrameSARTSolver``: the fp64 projections of the truths through the matrix as stored (``fit_forward``), with
``nrep`` noisy replicas each if asked, are cold columns of one batch.

The data are made with the matrix that solves them (an f16 shard projects with the quantised matrix): the study measures
the algorithm, its regularisation and the noise, not model error.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ..ops import hip
from .fit import fit_forward
from .sart import SolveResult
from .uncertainty import _device, perturbed_frames

SUM_NAMES = ("s_t", "s_x", "s_tt", "s_xx", "s_xt", "s_dd", "s_in", "m_d", "m_t", "m_x")
SCORE_NAMES = ("rel_l2", "cosine", "total_ratio", "peak_ratio", "max_error", "inside_fraction")
GROUP = 8  # columns per launch of the scoring kernel


def phantom_sums(X, t, device=None) -> np.ndarray:
    """``[nc, 10]`` (``SUM_NAMES``' order) for the columns ``X`` ``[nc, nvoxel]`` (or one column: ``[10]``) against the
    truth ``t`` ``[nvoxel]``, 8 columns per launch. A column's values depend on that column and the truth alone."""
    Xh = np.asarray(X, dtype=np.float64)
    one = Xh.ndim == 1
    Xh = np.ascontiguousarray(np.atleast_2d(Xh))
    th = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1))
    if Xh.ndim != 2 or Xh.shape[1] != th.size or th.size < 1:
        raise ValueError("X must be [nc, nvoxel] and t [nvoxel], nvoxel >= 1")
    nc, nvoxel = Xh.shape
    dev = _device(device)
    k = hip()
    out = np.empty((nc, len(SUM_NAMES)), dtype=np.float64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        td = torch.from_numpy(th).to(dev)
        sums = torch.empty((GROUP, len(SUM_NAMES)), dtype=torch.float64, device=dev)
        scratch = torch.empty(int(k.phantom64_scratch_elems(nvoxel)), dtype=torch.float64, device=dev)
        for c0 in range(0, nc, GROUP):
            n = min(GROUP, nc - c0)
            Xd = torch.from_numpy(Xh[c0: c0 + n]).to(dev)
            k.phantom64(Xd.data_ptr(), nvoxel, nvoxel, n, td.data_ptr(), sums.data_ptr(), scratch.data_ptr(), stream)
            out[c0: c0 + n] = sums[:n].cpu().numpy()
    return out[0] if one else out


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        return np.where(den == 0.0, np.nan, np.divide(num, den))


def phantom_scores(sums) -> Dict[str, np.ndarray]:
    """The six scores (``SCORE_NAMES``) from sums ``[..., 10]``, each of shape ``[...]``."""
    s = np.asarray(sums, dtype=np.float64)
    if s.shape[-1] != len(SUM_NAMES):
        raise ValueError("sums must be [..., 10]")
    v = {name: s[..., i] for i, name in enumerate(SUM_NAMES)}
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        rel_l2 = np.sqrt(_ratio(v["s_dd"], v["s_tt"]))
        norms = np.sqrt(v["s_xx"] * v["s_tt"])
    return {
        "rel_l2": rel_l2,
        "cosine": _ratio(v["s_xt"], norms),
        "total_ratio": _ratio(v["s_x"], v["s_t"]),
        "peak_ratio": _ratio(v["m_x"], v["m_t"]),
        "max_error": _ratio(v["m_d"], v["m_t"]),
        "inside_fraction": _ratio(v["s_in"], v["s_x"]),
    }


@dataclass
class PhantomResult:
    truth: np.ndarray               # [nvoxel]
    time: float
    image: np.ndarray               # [npixel] the noise-free projection A t (fp64, the matrix as stored)
    frames: np.ndarray              # [nrep + 1, npixel] what was solved (row 0: image)
    columns: List[SolveResult]      # [nrep + 1]
    sums: np.ndarray                # [nrep + 1, 10]
    scores: Dict[str, np.ndarray]   # each [nrep + 1]


def solve_phantoms(solver, truths, nrep: int = 0, times: Optional[Sequence[float]] = None, abs: float = 0.0,  # noqa: A002
                   shot: float = 0.0, rel: float = 0.0, seed: int = 0) -> List[PhantomResult]:
    """Every truth of ``truths`` ``[n, nvoxel]`` projected in fp64 through ``solver.rtm`` and solved, with ``nrep``
    noisy replicas each (0: none; the noise of ``perturbed_frames`` at the phantom's time, default 0, 1, ...), as cold
    columns of ``solve_batch`` on a ``MultiFrameSARTSolver`` (one rank); then the sums and scores of every column."""
    if solver.comm.world_size != 1:
        raise NotImplementedError("solve_phantoms runs on one rank (the native driver's --phantom takes several)")
    T = np.atleast_2d(np.asarray(truths, dtype=np.float64))
    if T.ndim != 2 or T.shape[0] < 1 or T.shape[1] != solver.rtm.nvoxel:
        raise ValueError(f"truths must be [n >= 1, {solver.rtm.nvoxel}]")
    if not np.all(np.isfinite(T)) or np.any(T < 0):
        raise ValueError("truths must be finite and >= 0")
    n = T.shape[0]
    tm = np.arange(n, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
    if tm.size != n or np.any(np.diff(tm) <= 0):
        raise ValueError("times must hold one strictly increasing entry per truth")
    if nrep < 0 or (nrep > 0 and (min(abs, shot, rel) < 0 or max(abs, shot, rel) <= 0)):
        raise ValueError("nrep must be >= 0, the noise terms >= 0 and, with replicas, one of them > 0")
    images = np.atleast_2d(fit_forward(solver.rtm, T))
    frames = [perturbed_frames(images[k], float(tm[k]), nrep, abs, shot, rel, seed, 0, device=solver.dev)
              for k in range(n)]
    nc = nrep + 1
    cols = solver.solve_batch(np.concatenate(frames, axis=0))
    out = []
    for k in range(n):
        ck = cols[k * nc: (k + 1) * nc]
        sums = phantom_sums(np.stack([c.solution for c in ck]), T[k], device=solver.dev)
        out.append(PhantomResult(T[k], float(tm[k]), images[k], frames[k], ck, sums, phantom_scores(sums)))
    return out
