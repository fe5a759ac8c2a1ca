"""Fit diagnostics: project solutions back through the RTM as stored and compare with the measured images.

``fit_forward(rtm, X)`` runs the fp64 fit kernels (csrc/kernels/fit64.hip) on a device shard -- ``DenseRTM`` in fp32,
bf16 or row-scaled f16 storage (row or column shard) or ``SparseRTM`` -- for any number of solutions, up to
``group_size(rtm)`` per pass over the matrix. Every product and sum is an fp64 FMA and widening the stored elements is
exact, so the images carry no rounding of the diagnostic's own; a value depends on its pixel row and its solution only,
not on how the solutions were grouped.

``fit_statistics`` (native, plain sequential loops) gives the residual norms over the pixels a solver uses: measured
value non-negative (negative pixels are saturated) and ray length above the threshold.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from ..ops import hip, native

def group_size(rtm) -> int:
    """Solutions per pass at which a frame costs least on this shard's storage (native ``fit64_group``: 8, and 4 on
    bf16 / f16 shards, where the fp64 FMAs of a wider pass cost more than the second read of the matrix)."""
    sparse = getattr(rtm, "nnz", None) is not None
    return int(hip().fit64_group(bool(getattr(rtm, "is_bf16", False)), bool(getattr(rtm, "is_f16", False)), sparse))


@dataclass
class FitResult:
    image: np.ndarray                    # f = A x over the statistics' pixels (fp64)
    residual_norm: float                 # sqrt(sum_S (g - f)^2)
    measurement_norm: float              # sqrt(sum_S g^2)
    residual_max: float                  # max_S |g - f|
    pixels: int                          # |S|
    residual_norm_camera: np.ndarray
    measurement_norm_camera: np.ndarray
    pixels_camera: np.ndarray

    @property
    def relative_residual(self) -> float:
        return self.residual_norm / self.measurement_norm if self.measurement_norm > 0 else float("nan")


def fit_forward(rtm, X, lanes: int = 0) -> np.ndarray:
    """``F[j] = A X[j]`` in fp64 for the shard ``rtm``: ``X`` is ``[nv, nvoxel]`` (or one vector) over this shard's
    voxels, the result ``[nv, npixel_local]`` (a column shard's partial images are to be summed over the shards).
    ``lanes``: lanes per row of the sparse kernel (4, 8, 16 or 32; 0: a fixed 8, whatever the shard, so that a row's
    bits do not depend on the row partition)."""
    Xh = np.asarray(X, dtype=np.float64)
    one = Xh.ndim == 1
    Xh = np.atleast_2d(Xh)
    if Xh.ndim != 2 or Xh.shape[1] != rtm.nvoxel:
        raise ValueError(f"X must be [nv, {rtm.nvoxel}] over the shard's voxels")
    nv, dev = Xh.shape[0], rtm.device
    sparse = getattr(rtm, "nnz", None) is not None
    ldx, ldf = int(rtm.ld), int(rtm.nrows_pad)
    out = np.empty((nv, rtm.npixel), dtype=np.float64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        group = group_size(rtm)
        Xd = torch.zeros((min(nv, group), ldx), dtype=torch.float64, device=dev)
        Fd = torch.zeros((min(nv, group), ldf), dtype=torch.float64, device=dev)
        Xt = torch.zeros((ldx, 8), dtype=torch.float64, device=dev) if sparse else None
        for j0 in range(0, nv, group):
            n = min(group, nv - j0)
            Xd[:n, : rtm.nvoxel].copy_(torch.from_numpy(Xh[j0: j0 + n]))
            fit_forward_device(rtm, Xd, n, Fd, Xt=Xt, lanes=lanes, stream=stream)
            out[j0: j0 + n] = Fd[:n, : rtm.npixel].cpu().numpy()
    return out[0] if one else out


def fit_forward_device(rtm, Xd: torch.Tensor, nv: int, Fd: torch.Tensor, Xt: Optional[torch.Tensor] = None,
                       lanes: int = 0, stream: int = 0) -> None:
    """One pass on device operands: ``Xd`` fp64 ``[>= nv, ldx]`` (``ldx >= rtm.ld``; entries at and beyond ``nvoxel``
    are not used), ``Fd`` fp64 ``[>= nv, ldf]`` (``ldf >= npixel``), ``Xt`` the sparse kernel's ``[ld, 8]`` scratch."""
    k = hip()
    if Xd.dtype != torch.float64 or Fd.dtype != torch.float64 or not Xd.is_contiguous() or not Fd.is_contiguous():
        raise ValueError("X and F must be contiguous float64 device tensors")
    if Xd.shape[0] < nv or Fd.shape[0] < nv:
        raise ValueError("X and F must hold nv rows")
    if getattr(rtm, "nnz", None) is not None:
        if Xt is None or Xt.dtype != torch.float64 or Xt.numel() < rtm.ld * 8:
            raise ValueError("the sparse fit kernel needs a float64 scratch of ld x 8 entries")
        k.fit_forward_csr(rtm.row_ptr.data_ptr(), rtm.col.data_ptr(), rtm.val.data_ptr(), rtm.nnz, rtm.npixel,
                          rtm.nvoxel, rtm.ld, Xd.data_ptr(), Xd.shape[1], nv, Xt.data_ptr(), Fd.data_ptr(),
                          Fd.shape[1], stream, lanes)
        return
    k.fit_forward(rtm.A.data_ptr(), rtm.ld, rtm.npixel, rtm.nrows_pad, rtm.nvoxel, Xd.data_ptr(), Xd.shape[1], nv,
                  Fd.data_ptr(), Fd.shape[1], stream, bf16=rtm.is_bf16, f16=rtm.is_f16,
                  rscale=rtm.row_scale.data_ptr() if rtm.is_f16 else 0)


def fit_statistics(f, g, ell, threshold: float, camera_pixels: Optional[Sequence[int]] = None) -> FitResult:
    """Residual statistics of the fitted image ``f`` against the measurement ``g`` over the pixels with ``g >= 0`` and
    ``ell > threshold``, in all and per camera (``camera_pixels``: pixels per camera in order; default one camera)."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    ell = np.ascontiguousarray(ell, dtype=np.float64)
    cams = [int(g.size)] if camera_pixels is None else [int(c) for c in camera_pixels]
    d = native().fit_statistics(f, g, ell, float(threshold), cams)
    return FitResult(image=f, residual_norm=float(d["residual_norm"]), measurement_norm=float(d["measurement_norm"]),
                     residual_max=float(d["residual_max"]), pixels=int(d["pixels"]),
                     residual_norm_camera=np.asarray(d["residual_norm_camera"]),
                     measurement_norm_camera=np.asarray(d["measurement_norm_camera"]),
                     pixels_camera=np.asarray(d["pixels_camera"]))
