#!/usr/bin/env python3
"""A Laplacian-weight scan against its alternatives, one session, on the ray-traced 64k x 64k matrix of the storage
benchmarks (tools/storage_bench.py), cold 20-update solves:

* (a) a 16-weight scan of one frame through ``MultiFrameSARTSolver(batch=16).solve_batch(betas=...)``;
* (b) ``solve_batch`` of 16 distinct frames at one scalar weight on the same build (the same kernels and bytes: only
  the penalty's weight load differs);
* (c) 16 single-frame ``SARTSolver`` solves (the fused sweep), one per weight -- what a scan cost before.

The cases alternate within the session (``--repeats`` rounds of ``--reps`` timed solves each after ``--warmup`` untimed
ones); the spread of a case's rounds is the run-to-run spread a difference has to exceed. JSON lines; the summary line
carries the ratios a/b (expected >= 0.85) and c/a (reported only). ``--root DIR --cases b`` runs case (b) against
another checkout of the package (the parent commit, which has no ``betas`` argument) for the scalar path's own A/B.

    python tools/beta_scan_bench.py --out profiles/beta_scan_64k.jsonl
    python tools/beta_scan_bench.py --nvox 4096 --cam 32x32 --reps 2          # a small shape

Host clock around ``solve_batch`` / ``solve`` (both return host arrays, i.e. end synchronised). Not measured:
multi-GPU, other batch widths, other storages, hardware counters (PMC).
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import the package from (default: this one)")
    ap.add_argument("--nvox", type=int, default=65536)
    ap.add_argument("--cam", default="128x256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5, help="timed solves per round")
    ap.add_argument("--repeats", type=int, default=3, help="rounds per case (alternating)")
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch

    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
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
    NB = 16
    betas = np.concatenate([[0.0], np.logspace(-5, -1, NB - 1)])
    scalar = float(betas[NB // 2])
    cases = [c for c in a.cases.split(",") if c]
    t0 = time.perf_counter()
    cam = tuple(int(v) for v in a.cam.split("x"))
    A, X, _, grid, _, rng = parity.raytraced_problem(a.nvox, cam, nframes=NB)
    rtm = DenseRTM.from_dense(A, device=dev)
    G = parity.frames_from(rtm.A[: rtm.npixel, : rtm.nvoxel], X, rng)
    P, V = A.shape
    del A
    L = LaplacianCSR.grid_3d(*grid, device=dev)
    kw = dict(max_iterations=a.steps, conv_tolerance=0.0)
    run = {}
    if "a" in cases:
        scan = MultiFrameSARTSolver(rtm, L, None, SolverParams(beta_laplace=0.0, **kw), batch=NB,
                                    allow_zero_tolerance=True, frame_betas=True)
        Ga = np.repeat(G[:1], NB, axis=0)
        run["a"] = lambda: scan.solve_batch(Ga, betas=betas)
    if "b" in cases:
        batch = MultiFrameSARTSolver(rtm, L, None, SolverParams(beta_laplace=scalar, **kw), batch=NB,
                                     allow_zero_tolerance=True)
        run["b"] = lambda: batch.solve_batch(G[:NB])
    if "c" in cases:
        # beta = 0 runs without a Laplacian, as a user's single run at that weight would
        singles = [SARTSolver(rtm, L if b > 0 else None, None, SolverParams(beta_laplace=float(b), **kw),
                              allow_zero_tolerance=True) for b in betas]
        run["c"] = lambda: [s.solve(G[0]) for s in singles]
    emit(dict(setup=True, tag=a.tag, shape=[P, V], grid=list(grid),
              steps=a.steps, warmup=a.warmup, reps=a.reps, repeats=a.repeats, weights=NB, cases=cases,
              seconds=time.perf_counter() - t0, device=torch.cuda.get_device_name(dev),
              timing="host clock around solves that return host arrays; cases alternate within the session",
              not_measured="multi-GPU, other batch widths and storages, hardware counters (PMC)"))
    for c in cases:
        for _ in range(a.warmup):
            run[c]()
    sec = {c: [] for c in cases}
    for rnd in range(a.repeats):
        for c in cases:
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            for _ in range(a.reps):
                out = run[c]()
            torch.cuda.synchronize(dev)
            s = (time.perf_counter() - t) / a.reps
            sec[c].append(s)
            emit(dict(tag=a.tag, case=c, round=rnd, ms_per_scan=1e3 * s, column_it_per_s=NB * a.steps / s,
                      used_fused=bool(out[0].used_fused), iterations=int(out[0].iterations)))
    med = {c: float(np.median(v)) for c, v in sec.items()}
    summary = dict(summary=True, tag=a.tag, shape=[P, V], steps=a.steps,
                   ms_median={c: 1e3 * med[c] for c in cases},
                   column_it_per_s={c: NB * a.steps / med[c] for c in cases},
                   spread={c: (max(v) - min(v)) / med[c] for c, v in sec.items()})
    if "a" in med and "b" in med:
        summary.update(a_over_b=med["b"] / med["a"], expected_at_least=0.85)  # rates: (a) / (b)
    if "a" in med and "c" in med:
        summary.update(c_over_a=med["c"] / med["a"])  # times: 16 single solves over one scan
    emit(summary)


if __name__ == "__main__":
    main()
