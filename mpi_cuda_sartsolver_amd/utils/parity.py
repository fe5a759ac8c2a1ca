"""Parity of every default solver path at a production shape, against the device fp64 oracle.

The reference multiplies raw fp32 RTM values with plain FMAs (reference sart_kernels.cu:63-110) on production
matrices -- ray-traced with wall reflections (default dataset ``with_reflections``, arguments.cpp:135-137), entries
over many decades, most of them zero. The host fp32 emulation (models/reference.py) is too slow beyond ~4k x 8k, so
at scale the fp32 yardstick is the fp32 two-pass kernels on the same shard: each path's relative error against the
fp64 oracle (models/oracle.py: the same algorithm in fp64 on the device) is compared with the two-pass kernels'
error on the same frame, iteration count and variant ("ratio"; the two-pass kernels are plain fp32 dot products and
split-K sums, the reference's own arithmetic class).

Paths: the fused sweep, the two-pass kernels and the column (voxel) shard; linear / log, with / without the
Laplacian; the multi-frame engine at 32 / 64 / 128 frames (split-A on range-safe f16 pairs); bf16 storage (fused, and
multi-frame at 64, against the oracle and two-pass kernels of the bf16-rounded matrix); and the no-reflection part
held sparse (CSR / CSC two-pass kernels, multi-frame SpMM), against the oracle of the same matrix held dense.

Used by tools/parity_at_scale.py (64k x 64k, profiles/parity_r6_64k_raytraced.jsonl) and tests/test_gpu_parity.py
(a 16k x 16k shard in the suite).
"""
from __future__ import annotations

import time
from typing import Callable, Dict, Iterable, List, Optional

import numpy as np

GRIDS = {4096: (16, 16, 16), 16384: (16, 32, 32), 32768: (32, 32, 32), 65536: (32, 32, 64),
         327680: (64, 64, 80)}


def raytraced_problem(nvox: int, cam_shape, nframes: int = 128, seed: int = 3, keep_direct: bool = False):
    """(A fp32 [2 cameras x pixels, nvox], G [nframes, pixels] fp64 from the drifting phantom (2 % saturated pixels),
    info) of utils/raytrace.py's ray-traced model with reflections."""
    from .raytrace import Camera, default_cameras, phantom, raytraced_rtm

    grid = GRIDS[nvox]
    cams = [Camera(c, bc.position, bc.look_at, tuple(cam_shape), bc.field_of_view, bc.up)
            for c, bc in zip(("cam_a", "cam_b"), default_cameras(n=2))]
    A, info = raytraced_rtm(grid=grid, cameras=cams, keep_direct=keep_direct)
    rng = np.random.default_rng(seed)
    X = np.stack([phantom(grid, t=0.1 * t) for t in range(nframes)])
    return A, X, cams, grid, info, rng


def frames_from(A_dev, X, rng, saturate: float = 0.02):
    """G = A X^T on the device (fp64 out), saturated pixels -1."""
    import torch

    Xd = torch.from_numpy(X.T.astype(np.float32)).to(A_dev.device)
    G = (A_dev @ Xd).double().cpu().numpy().T.copy()
    G[rng.random(G.shape) < saturate] = -1.0
    return G


def _rel(a, b) -> float:
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run(A: np.ndarray, G: np.ndarray, dev, *, iters: Iterable[int] = (1, 20), frames=(0, 1), beta: float = 1e-3,
        laplacian=None, batches=(32, 64, 128), variants=None, bf16: bool = True, column_shard: bool = True,
        sparse_A: Optional[np.ndarray] = None, emit: Callable[[Dict], None] = print, tag: str = "",
        single: bool = True, oracle: str = "torch") -> List[Dict]:
    """Every path x variant x iteration count; one record per (path, variant, iterations, frame).
    oracle: "torch" (models/oracle.py, the default) or "native": the double-precision engine (SARTSolver with
    precision="fp64", gpu semantics, tolerance 0, fixed iterations) where it reads the shard (fp32 dense); bf16-stored
    shards keep the torch loop, which dequantises them."""
    import torch

    from ..models.multiframe import MultiFrameSARTSolver
    from ..models.oracle import sart_oracle_f64
    from ..models.rtm import DenseRTM, SparseRTM
    from ..models.sart import SARTSolver, SolverParams

    if oracle not in ("torch", "native"):
        raise ValueError("oracle must be 'torch' or 'native'")
    torch_oracle = sart_oracle_f64

    def sart_oracle_f64(r, g, it, logarithmic=False, laplacian=None, beta_laplace=0.0):  # noqa: F811
        if oracle == "native" and not r.is_16bit:
            s = SARTSolver(r, laplacian, None, SolverParams(max_iterations=it, conv_tolerance=0.0,
                                                            beta_laplace=beta_laplace if laplacian is not None else 1e-2),
                           logarithmic=logarithmic, allow_zero_tolerance=True, precision="fp64", semantics="gpu")
            return s.solve(g).solution
        return torch_oracle(r, g, it, logarithmic=logarithmic, laplacian=laplacian, beta_laplace=beta_laplace)

    out: List[Dict] = []
    P, V = A.shape
    rtm = DenseRTM.from_dense(A, device=dev)
    variants = variants or [(log, lap) for log in (False, True) for lap in (False, True)]

    def record(path, log, lap, it, f, x, x64, e_ref, factor, extra=None):
        e = _rel(x, x64)
        rec = dict(tag=tag, shape=[P, V], path=path, log=log, laplacian=lap, iterations=it, frame=f, err=e,
                   err_two_pass=e_ref, ratio=e / e_ref if e_ref > 0 else None, bound=factor,
                   ok=bool(e <= factor * e_ref + 1e-9), **(extra or {}))
        out.append(rec)
        emit(rec)
        return rec

    def solver(r, log, L, it, **kw):
        return SARTSolver(r, L, None, SolverParams(max_iterations=it, conv_tolerance=0.0, beta_laplace=beta),
                          logarithmic=log, allow_zero_tolerance=True, **kw)

    def mf(r, log, L, it, batch):
        return MultiFrameSARTSolver(r, L, None, SolverParams(max_iterations=it, conv_tolerance=0.0, beta_laplace=beta),
                                    logarithmic=log, batch=batch, allow_zero_tolerance=True)

    for log, lapv in variants:
        L = laplacian if lapv else None
        for it in iters:
            t0 = time.perf_counter()
            ref = {}
            for f in frames:
                x64 = sart_oracle_f64(rtm, G[f], it, logarithmic=log, laplacian=L, beta_laplace=beta)
                xtp = solver(rtm, log, L, it, use_fused=False).solve(G[f]).solution
                ref[f] = (x64, _rel(xtp, x64))
                record("two_pass", log, lapv, it, f, xtp, x64, ref[f][1], 1.0)
                if not single:
                    continue
                s = solver(rtm, log, L, it, use_fused=True)
                g = s.geom
                record("fused", log, lapv, it, f, s.solve(G[f]).solution, x64, ref[f][1], FACTORS["fused"],
                       dict(geometry=None if g is None else dict(T=g.T, kw=g.kw, I=g.I, J=g.J)))
                if column_shard and not lapv:
                    xc = solver(rtm, log, L, it, partition="cols").solve(G[f]).solution
                    record("column_shard", log, lapv, it, f, xc, x64, ref[f][1], FACTORS["column_shard"])
            for batch in batches:
                m = mf(rtm, log, L, it, batch)
                res = m.solve_batch(G[:batch])
                for f in frames:
                    record(f"multiframe{batch}", log, lapv, it, f, res[f].solution, ref[f][0], ref[f][1],
                           FACTORS["multiframe"], dict(split=[m.forward_split, m.backproject_split]))
                del m
            emit(dict(tag=tag, timing=True, log=log, laplacian=lapv, iterations=it, seconds=time.perf_counter() - t0))
    if bf16:  # exact SART of the bf16-rounded matrix: oracle and two-pass yardstick on that matrix
        r16 = rtm.to_bf16()
        for log in (False, True):
            for it in iters:
                for f in frames:
                    x64 = sart_oracle_f64(r16, G[f], it, logarithmic=log)
                    xtp = solver(r16, log, None, it, use_fused=False).solve(G[f]).solution
                    e_tp = _rel(xtp, x64)
                    record("bf16_two_pass", log, False, it, f, xtp, x64, e_tp, 1.0)
                    record("bf16_fused", log, False, it, f, solver(r16, log, None, it, use_fused=True).solve(G[f]).solution,
                           x64, e_tp, FACTORS["bf16_fused"])
                res = mf(r16, log, None, it, 64).solve_batch(G[:64])
                for f in frames:
                    x64 = sart_oracle_f64(r16, G[f], it, logarithmic=log)
                    e_tp = _rel(solver(r16, log, None, it, use_fused=False).solve(G[f]).solution, x64)
                    record("bf16_multiframe64", log, False, it, f, res[f].solution, x64, e_tp, FACTORS["bf16_multiframe"])
        del r16
    if sparse_A is not None:  # the no-reflection part held sparse, against the oracle of the same matrix held dense
        del rtm
        torch.cuda.empty_cache()
        rd = DenseRTM.from_dense(sparse_A, device=dev)
        sp = SparseRTM.from_dense(sparse_A, device=dev)
        Gd = G  # (frames of the full model: a different measurement, the same comparison)
        for log in (False, True):
            for it in iters:
                for f in frames:
                    x64 = sart_oracle_f64(rd, Gd[f], it, logarithmic=log)
                    e_tp = _rel(solver(rd, log, None, it, use_fused=False).solve(Gd[f]).solution, x64)
                    record("sparse_two_pass", log, False, it, f, solver(sp, log, None, it).solve(Gd[f]).solution, x64,
                           e_tp, FACTORS["sparse"])
                res = mf(sp, log, None, it, 64).solve_batch(Gd[:64])
                for f in frames:
                    x64 = sart_oracle_f64(rd, Gd[f], it, logarithmic=log)
                    e_tp = _rel(solver(rd, log, None, it, use_fused=False).solve(Gd[f]).solution, x64)
                    record("sparse_multiframe64", log, False, it, f, res[f].solution, x64, e_tp, FACTORS["sparse"])
    return out


# Bounds, as multiples of the fp32 two-pass kernels' error on the same frame (see the module docstring), set from the
# 64k x 64k measurement (profiles/parity_r6_64k_raytraced.jsonl):
#   fused / column shard / sparse: other fp32 summation orders of the same products (segmented chains, per-column
#     sums, CSR gathers): measured 0.84 - 1.14x, bound 1.25x;
#   multiframe: fp32 MFMA (16 frames) or range-safe f16 pairs (2^-22 per product, 32 - 128 frames) with two-level
#     split-K accumulation (round 6: one fp32 MFMA chain per 16k-term split measured 3.5 - 9.8x): measured
#     0.74 - 1.14x, bound 1.25x;
#   bf16 storage: the bf16 matrix is exact; the fused bf16 tiles carry x as bf16 hi + lo pieces (2^-17: measured
#     2.8 - 4.1x) and the bf16 MFMA kernels X / W as bf16 hi + lo (2^-17) -- documented factors 5x and 12x.
FACTORS = {"fused": 1.25, "column_shard": 1.25, "multiframe": 1.25, "bf16_fused": 5.0, "bf16_multiframe": 12.0,
           "sparse": 1.25}
