#!/usr/bin/env python3
"""The double-precision engine (``SARTSolver(precision="fp64")``, sart::Engine64) next to the fp32 paths, on one matrix
in one session: it/s of the fp64 two-pass sweep, of the fp32 two-pass kernels (the yardstick: both read the matrix
twice per iteration) and of the fp32 fused sweep, with fixed iterations (``--steps`` updates per cold solve, tolerance
0, ``--warmup`` untimed solves first), as tools/storage_bench.py. Then the fp64 solution's distance from the fp32
fused, bf16 and f16 solutions of the same frame (what one reads off when judging a storage format), and from the torch
fp64 loop (models/oracle.py). JSON lines; the matrix is the ray-traced 64k x 64k one of tools/storage_bench.py.

    python tools/fp64_bench.py --out profiles/fp64_engine_64k.jsonl
    python tools/fp64_bench.py --nvox 4096 --cam 32x32 --steps 10      # a small shape
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvox", type=int, default=65536, help="voxels (a grid of utils/parity.py GRIDS)")
    ap.add_argument("--cam", default="128x256", help="pixels per camera (two cameras)")
    ap.add_argument("--steps", type=int, default=20, help="SART updates per solve (fixed)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2, help="timed solves per path")
    ap.add_argument("--log", action="store_true", help="the logarithmic solver too")
    ap.add_argument("--no-distances", action="store_true", help="rates only")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file (default: stdout only)")
    a = ap.parse_args()
    import torch

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
    t0 = time.perf_counter()
    cam = tuple(int(v) for v in a.cam.split("x"))
    A, X, _, grid, _, rng = parity.raytraced_problem(a.nvox, cam, nframes=1)
    base = DenseRTM.from_dense(A, device=dev)
    g = parity.frames_from(base.A[: base.npixel, : base.nvoxel], X, rng)[0]
    P, V = A.shape
    del A
    emit(dict(setup=True, tag=a.tag, shape=[P, V], grid=list(grid), cams=list(cam), steps=a.steps, warmup=a.warmup,
              reps=a.reps, seconds=time.perf_counter() - t0, rtm="ray-traced with reflections (utils/raytrace.py)",
              device=torch.cuda.get_device_name(dev),
              not_measured="multi-GPU, other widths, hardware counters (PMC)"))
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
        common = dict(tag=a.tag, shape=[P, V], log=log, steps=a.steps, shard_GB=base.nbytes / 1e9)
        rates, sols = {}, {}
        for name, kw in (("fp64 two-pass", dict(precision="fp64", semantics="gpu")),
                         ("fp32 two-pass", dict(use_fused=False)), ("fp32 fused", dict(use_fused=True))):
            s = SARTSolver(base, None, None, params, logarithmic=log, allow_zero_tolerance=True, **kw)
            r, sec = timed(lambda: s.solve(g))
            reads = 1 if r.used_fused else 2
            rates[name], sols[name] = a.steps / sec, r.solution
            emit(dict(common, path=name, used_fused=bool(r.used_fused), it_per_s=a.steps / sec, ms_per_solve=1e3 * sec,
                      rtm_TBps=reads * base.nbytes * a.steps / sec / 1e12))
            del s
        emit(dict(common, summary=True, fp64_it_per_s=rates["fp64 two-pass"], fp32_two_pass_it_per_s=rates["fp32 two-pass"],
                  fp32_fused_it_per_s=rates["fp32 fused"],
                  fp64_over_fp32_two_pass=rates["fp64 two-pass"] / rates["fp32 two-pass"]))
        if a.no_distances:
            continue
        x64 = sols["fp64 two-pass"]
        dist = {"fp32 fused": rel(sols["fp32 fused"], x64), "fp32 two-pass": rel(sols["fp32 two-pass"], x64)}
        for storage, kws in (("bf16", [("bf16", {})]), ("f16", [("f16 two-pass", {}), ("f16 fused", dict(f16_fused=True))])):
            rtm = base.to_bf16() if storage == "bf16" else base.to_f16()
            for name, kw in kws:
                s = SARTSolver(rtm, None, None, params, logarithmic=log, allow_zero_tolerance=True, **kw)
                dist[name] = rel(s.solve(g).solution, x64)
                del s
            del rtm
            torch.cuda.empty_cache()
        t1 = time.perf_counter()
        dist["torch fp64 oracle"] = rel(sart_oracle_f64(base, g, a.steps, logarithmic=log), x64)
        emit(dict(common, distances_from_fp64_engine=dist, oracle_seconds=time.perf_counter() - t1,
                  metric="||x - x_fp64|| / ||x_fp64|| after %d updates" % a.steps))


if __name__ == "__main__":
    main()
