"""L-curve of a Laplacian-weight scan: every frame solved at a ladder of weights in one batch, the residual norm
against the roughness norm per weight, and the curve's corner.

``roughness(L, X)`` runs the fp64 roughness kernel (csrc/kernels/rough64.hip): ``sqrt(sum_r (L u)_r^2)`` with ``u = x``
or ``log(max(x, 1e-100))``, up to 8 solutions per pass over the Laplacian, every product and sum an fp64 FMA, no
atomics -- a value depends on its solution only, not on how the solutions were grouped or on the run.
``lcurve_corner`` is the native corner rule (csrc/native/lcurve.cpp): the largest positive Menger curvature of
``(log rho, log eta)`` over the weights in increasing order. ``beta_scan`` puts them together on a
``MultiFrameSARTSolver``: the weights are columns of the batch engine (``solve_batch(betas=...)``), so a ladder costs
about one batched sweep per iteration instead of one single-frame sweep per weight.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch

from ..ops import hip, native
from .fit import fit_forward, fit_statistics
from .laplacian import LaplacianCSR
from .sart import SolveResult

GROUP = 8  # solutions per pass of the roughness kernel


def roughness_squared(L: LaplacianCSR, X, log: bool = False, device=None) -> np.ndarray:
    """``eta2[j] = sum_{r < n} (sum_k L[r, k] u_j[k])^2`` in fp64 on the GPU, as the kernel returns it. ``X``:
    ``[nv, >= n]`` (or one vector); entries at and beyond ``L.n`` are never read. A Laplacian kept on the host is
    uploaded to ``device`` (default: the current GPU) for the call."""
    Xh = np.asarray(X, dtype=np.float64)
    one = Xh.ndim == 1
    Xh = np.ascontiguousarray(np.atleast_2d(Xh))
    if Xh.ndim != 2 or Xh.shape[1] < L.n:
        raise ValueError(f"X must be [nv, >= {L.n}] over the Laplacian's voxels")
    dev = L.device
    if dev is not None and dev.type == "cuda":
        rp, col, val = L.row_ptr, L.col, L.val
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        rp, col, val = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                        for a in (L.row_ptr_host, L.col_host, L.val_host))
    k = hip()
    nv, ldx = Xh.shape
    out = np.empty(nv, dtype=np.float64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        scratch = torch.zeros(int(k.rough64_scratch_elems(L.n)), dtype=torch.float64, device=dev)
        eta2 = torch.zeros(GROUP, dtype=torch.float64, device=dev)
        for j0 in range(0, nv, GROUP):
            n = min(GROUP, nv - j0)
            Xd = torch.from_numpy(Xh[j0: j0 + n]).to(dev)
            k.rough64(rp.data_ptr(), col.data_ptr(), val.data_ptr(), L.n, Xd.data_ptr(), ldx, n, bool(log),
                      eta2.data_ptr(), scratch.data_ptr(), stream)
            out[j0: j0 + n] = eta2[:n].cpu().numpy()
    return out[0] if one else out


def roughness(L: LaplacianCSR, X, log: bool = False, device=None) -> np.ndarray:
    """Roughness norms ``sqrt(sum_r (L u)_r^2)`` of the solutions ``X`` (``u = x``, or ``log(max(x, 1e-100))`` with
    ``log``: the logarithmic solver's regulariser)."""
    return np.sqrt(roughness_squared(L, X, log, device))


def lcurve_corner(rho, eta, ok=None, fallback: int = 0) -> Tuple[int, bool, np.ndarray]:
    """``(selected, found, curvature)`` of the points ``(rho[i], eta[i])`` in increasing-weight order. A point counts
    when ``ok[i]`` and both norms are finite and > 0; ``curvature`` is NaN where undefined. ``selected`` is the point of
    largest curvature > 0 (ties: the smaller index), else ``fallback`` (the nearest valid point when it is not one)."""
    rho = np.ascontiguousarray(rho, dtype=np.float64).ravel()
    eta = np.ascontiguousarray(eta, dtype=np.float64).ravel()
    okv = np.ones(rho.size, dtype=np.uint8) if ok is None else np.ascontiguousarray(np.asarray(ok) != 0, dtype=np.uint8)
    sel, found, curv = native().lcurve_corner(rho, eta, okv.ravel(), int(fallback))
    return int(sel), bool(found), np.asarray(curv)


@dataclass
class ScanResult:
    betas: np.ndarray            # [nb] the ladder
    results: List[SolveResult]   # per frame: the selected weight's solve
    columns: List[List[SolveResult]]  # [T][nb] every solve
    residual_norm: np.ndarray    # [T, nb] sqrt(sum_S (g - A x)^2), A as stored
    roughness_norm: np.ndarray   # [T, nb]
    curvature: np.ndarray        # [T, nb], NaN where undefined
    selected: np.ndarray         # [T] index into betas
    corner_found: np.ndarray     # [T] bool


def beta_scan(solver, measurements, betas, fallback: int = 0) -> ScanResult:
    """Every frame of ``measurements`` ``[T, npixel]`` at every weight of ``betas`` (increasing) on a
    ``MultiFrameSARTSolver`` built with its Laplacian and ``frame_betas=True`` (one rank): ``T nb`` cold columns
    through ``solve_batch(betas=...)``, residual norms through the fit kernels on the matrix as stored (the pixel set of
    ``fit_statistics``), roughness norms through ``roughness``, and the corner per frame."""
    if solver.L is None:
        raise ValueError("beta_scan needs a solver built with a Laplacian (frame_betas=True)")
    if solver.comm.size != 1:
        raise NotImplementedError("beta_scan runs on one rank (the native driver's --beta_scan takes several)")
    b = np.asarray(betas, dtype=np.float64).ravel()
    if b.size < 3 or not np.all(np.isfinite(b)) or b[0] < 0 or not np.all(np.diff(b) > 0):
        raise ValueError("betas must be at least 3 increasing values >= 0")
    G = np.atleast_2d(np.asarray(measurements, dtype=np.float64))
    T, nb = G.shape[0], b.size
    cols = solver.solve_batch(np.repeat(G, nb, axis=0), betas=np.tile(b, T))
    X = np.stack([r.solution for r in cols])
    F = fit_forward(solver.rtm, X)
    ell = fit_forward(solver.rtm, np.ones(solver.rtm.nvoxel))
    thr = solver.params.ray_length_threshold
    rho = np.array([fit_statistics(F[j], G[j // nb], ell, thr).residual_norm for j in range(T * nb)]).reshape(T, nb)
    eta = roughness(solver.L, X, log=solver.log, device=solver.dev).reshape(T, nb)
    ok = np.array([not r.nonfinite for r in cols], dtype=np.uint8).reshape(T, nb)
    curv = np.full((T, nb), np.nan)
    sel = np.zeros(T, dtype=np.int32)
    found = np.zeros(T, dtype=bool)
    for k in range(T):
        sel[k], found[k], curv[k] = lcurve_corner(rho[k], eta[k], ok[k], fallback)
    columns = [cols[k * nb: (k + 1) * nb] for k in range(T)]
    return ScanResult(b, [columns[k][sel[k]] for k in range(T)], columns, rho, eta, curv, sel, found)
