#!/usr/bin/env python3
"""RTM storage formats side by side on one shape: fp32, bf16 and row-scaled f16 (``DenseRTM(storage=...)``).

``bench.py`` measures the flagship workload and has no f16 storage; this tool carries the storage comparison. On the
ray-traced RTM with reflections (utils/raytrace.py; the 64k x 64k matrix of tools/parity_at_scale.py by default) it
reports, per storage format, as JSON lines:

* single-frame it/s through ``SARTSolver`` on its default path (fused sweep; two-pass kernels for f16), on the
  two-pass kernels, and for f16 on the opt-in fused sweep (``f16_fused=True``), and multi-frame frame-it/s through ``MultiFrameSARTSolver`` at each ``--frames`` batch width,
  with fixed iterations (``--steps`` updates per solve, tolerance 0, ``--warmup`` untimed solves first), as bench.py;
* each path's relative error after ``--steps`` updates against the device fp64 oracle (``sart_oracle_f64``) on its
  OWN stored matrix (the arithmetic error of the path) and on the fp32 matrix (arithmetic + storage rounding).

    python tools/storage_bench.py --out storage_f16_64k.jsonl
    python tools/storage_bench.py --nvox 4096 --cam 32x32 --frames 16,64 --steps 10      # a small shape
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvox", type=int, default=65536, help="voxels (a grid of utils/parity.py GRIDS)")
    ap.add_argument("--cam", default="128x256", help="pixels per camera (two cameras)")
    ap.add_argument("--storages", default="fp32,bf16,f16")
    ap.add_argument("--frames", default="64,128", help="multi-frame batch widths")
    ap.add_argument("--steps", type=int, default=20, help="SART updates per solve (fixed)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2, help="timed solves per path")
    ap.add_argument("--log", action="store_true", help="the logarithmic solver too")
    ap.add_argument("--no-errors", action="store_true", help="rates only (no fp64 oracle runs)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file (default: stdout only)")
    a = ap.parse_args()
    import torch

    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.oracle import sart_oracle_f64
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
    from mpi_cuda_sartsolver_amd.utils import parity

    outf = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        outf = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()

    dev = torch.device("cuda", 0)
    widths = [int(v) for v in a.frames.split(",") if v]
    t0 = time.perf_counter()
    cam = tuple(int(v) for v in a.cam.split("x"))
    A, X, _, grid, _, rng = parity.raytraced_problem(a.nvox, cam, nframes=max(widths + [1]))
    base = DenseRTM.from_dense(A, device=dev)
    G = parity.frames_from(base.A[: base.npixel, : base.nvoxel], X, rng)
    P, V = A.shape
    del A
    emit(dict(setup=True, tag=a.tag, shape=[P, V], grid=list(grid), cams=list(cam), steps=a.steps, warmup=a.warmup,
              reps=a.reps, seconds=time.perf_counter() - t0, rtm="ray-traced with reflections (utils/raytrace.py)",
              device=torch.cuda.get_device_name(dev)))
    params = SolverParams(max_iterations=a.steps, conv_tolerance=0.0)
    rel = parity._rel

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        for _ in range(a.reps):
            out = fn()
        torch.cuda.synchronize(dev)
        return out, (time.perf_counter() - t) / a.reps

    for log in ([False, True] if a.log else [False]):
        x64_fp32 = None if a.no_errors else sart_oracle_f64(base, G[0], a.steps, logarithmic=log)
        for storage in a.storages.split(","):
            rtm = base if storage == "fp32" else (base.to_bf16() if storage == "bf16" else base.to_f16())
            x64_own = x64_fp32 if storage == "fp32" else (
                None if a.no_errors else sart_oracle_f64(rtm, G[0], a.steps, logarithmic=log))
            common = dict(tag=a.tag, shape=[P, V], storage=storage, log=log, steps=a.steps, shard_GB=rtm.nbytes / 1e9)
            if storage == "f16":
                common.update(f16_flushed=rtm.flushed_count,
                              f16_flushed_fraction=rtm.flushed_count / max(1, rtm.nonzero_count))

            def errors(x):
                if a.no_errors:
                    return {}
                return dict(err_own_matrix=rel(x, x64_own), err_fp32_matrix=rel(x, x64_fp32))

            fused_default = False
            paths = [("default", {}), ("two_pass", dict(use_fused=False))]
            if storage == "f16":
                paths.append(("f16_fused", dict(f16_fused=True)))  # the opt-in fused f16 sweep, next to the default
            for name, kw in paths:
                if name == "two_pass" and not fused_default:
                    continue  # the default path already was the two-pass kernels
                s = SARTSolver(rtm, None, None, params, logarithmic=log, allow_zero_tolerance=True, **kw)
                r, sec = timed(lambda: s.solve(G[0]))
                fused_default = bool(r.used_fused) if name == "default" else fused_default
                emit(dict(common, path="single-frame " + ("fused" if r.used_fused else "two-pass"), frames=1,
                          opt_in=name == "f16_fused", fallbacks=r.fallbacks, it_per_s=a.steps / sec, ms_per_solve=1e3 * sec,
                          rtm_TBps=(1 if r.used_fused else 2) * rtm.nbytes * a.steps / sec / 1e12, **errors(r.solution)))
                del s
            for nf in widths:
                m = MultiFrameSARTSolver(rtm, None, None, params, logarithmic=log, batch=nf, allow_zero_tolerance=True)
                res, sec = timed(lambda: m.solve_batch(G[:nf]))
                emit(dict(common, path=f"multi-frame {m.forward_split} / {m.backproject_split}", frames=nf,
                          batch_width=m.batch_width, frame_it_per_s=nf * a.steps / sec, ms_per_batch=1e3 * sec,
                          rtm_TBps=2 * rtm.nbytes * a.steps / sec / 1e12, **errors(res[0].solution)))
                del m
            if rtm is not base:
                del rtm
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
