#!/usr/bin/env python3
"""Hold-out columns against a batch of distinct frames, one session, on the ray-traced 64k x 64k matrix of the storage
benchmarks (tools/storage_bench.py), cold 20-update solves with the grid's Laplacian:

* (a) one frame at 4 Laplacian weights x (3 pixel folds + 1) = 16 columns through ``models.holdout.solve_holdout``: the
  masks, ``MultiFrameSARTSolver(batch=16).solve_batch`` of the 16 columns with a weight per column, then the fp64
  projections of the columns (``fit_forward_device``, two passes of 8 and one for the ray lengths), the scoring kernel
  and the scores;
* (b) ``solve_batch`` of 16 distinct ordinary frames on the same solver with the same weight per column: the same
  kernels and bytes, only the frames and the scoring pass differ.

The cases alternate within the session (``--repeats`` rounds of ``--reps`` timed solves each after ``--warmup`` untimed
ones); the spread of a case's rounds is the run-to-run spread a difference has to exceed. JSON lines; the summary line
carries the ratio a/b of the column-iterations per second (expected >= 0.85). A ``kernels`` line times the scoring
kernel alone (8 columns of all pixels in 4 cameras: device events around one launch, median of ``--kernel-reps``), and a
``curve`` line prints ``cv_error`` and ``train_error`` of a 16-weight ladder on the same frame (not asserted).

    python tools/holdout_bench.py --out profiles/holdout_64k.jsonl
    python tools/holdout_bench.py --nvox 4096 --cam 32x32 --reps 2          # a small shape

Host clock around calls that return host arrays (i.e. end synchronised). Not measured: multi-GPU runs, other batch
widths and storages, the native driver's hold-out pass at size (its reads of the stored columns and the host
all-reduce), hardware counters (PMC).
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvox", type=int, default=65536)
    ap.add_argument("--cam", default="128x256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5, help="timed solves per round")
    ap.add_argument("--repeats", type=int, default=3, help="rounds per case (alternating)")
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from mpi_cuda_sartsolver_amd.models.holdout import solve_holdout
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams
    from mpi_cuda_sartsolver_amd.ops import hip
    from mpi_cuda_sartsolver_amd.utils import parity
    from mpi_cuda_sartsolver_amd.utils.holdout import folds

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
    NC, K = 16, 3
    betas = np.array([0.0, 1e-4, 1e-3, 1e-2])
    ladder16 = np.concatenate([[0.0], np.logspace(-6, -1, 15)])
    t0 = time.perf_counter()
    cam = tuple(int(v) for v in a.cam.split("x"))
    A, X, _, grid, _, rng = parity.raytraced_problem(a.nvox, cam, nframes=NC)
    rtm = DenseRTM.from_dense(A, device=dev)
    G = parity.frames_from(rtm.A[: rtm.npixel, : rtm.nvoxel], X, rng)
    P, V = A.shape
    del A
    L = LaplacianCSR.grid_3d(*grid, device=dev)
    solver = MultiFrameSARTSolver(rtm, L, None, SolverParams(beta_laplace=1e-3, max_iterations=a.steps,
                                                             conv_tolerance=0.0),
                                  batch=NC, allow_zero_tolerance=True, frame_betas=True)
    cams = [P // 2, P - P // 2]
    f = folds(P, K, a.seed)
    col_betas = np.repeat(betas, K + 1)

    run = {"a": lambda: solve_holdout(solver, G[0], f, K, betas=betas, camera_pixels=cams).columns[0],
           "b": lambda: solver.solve_batch(G[:NC], betas=col_betas)}
    cases = ["a", "b"]
    emit(dict(setup=True, tag=a.tag, shape=[P, V], grid=list(grid), steps=a.steps, warmup=a.warmup, reps=a.reps,
              repeats=a.repeats, columns=NC, folds=K, betas=betas.tolist(), seed=a.seed,
              seconds=time.perf_counter() - t0, device=torch.cuda.get_device_name(dev),
              forward_split=solver.forward_split,
              timing="host clock around calls that return host arrays; cases alternate within the session",
              not_measured="multi-GPU runs, other batch widths and storages, the native driver's hold-out pass at "
                           "size, hardware counters (PMC)"))
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
            emit(dict(tag=a.tag, case=c, round=rnd, ms_per_batch=1e3 * s, column_it_per_s=NC * a.steps / s,
                      iterations=int(out[0].iterations)))
    med = {c: float(np.median(v)) for c, v in sec.items()}
    emit(dict(summary=True, tag=a.tag, shape=[P, V], steps=a.steps, ms_median={c: 1e3 * med[c] for c in cases},
              column_it_per_s={c: NC * a.steps / med[c] for c in cases},
              spread={c: (max(v) - min(v)) / med[c] for c, v in sec.items()},
              a_over_b=med["b"] / med["a"], expected_at_least=0.85))  # rates: (a) / (b)

    # the scoring kernel alone: 8 columns of all pixels in 4 cameras
    k = hip()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        gd = torch.from_numpy(G[0]).to(dev)
        Fd = (gd.clamp(min=0.0)[None, :] * torch.linspace(0.9, 1.1, 8, dtype=torch.float64, device=dev)[:, None]).contiguous()
        ell = torch.ones(P, dtype=torch.float64, device=dev)
        fd = torch.from_numpy(f).to(dev)
        held = torch.from_numpy(np.resize(np.arange(-1, K, dtype=np.int32), 8)).to(dev)
        starts = torch.from_numpy(np.linspace(0, P, 5).astype(np.int64)).to(dev)
        sums = torch.empty((8, 4, 6), dtype=torch.float64, device=dev)
        ms = []
        for i in range(a.kernel_reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            k.holdout64(Fd.data_ptr(), P, 8, gd.data_ptr(), ell.data_ptr(), 1e-6, fd.data_ptr(), held.data_ptr(),
                        starts.data_ptr(), 4, sums.data_ptr(), stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            if i:  # the first launch loads the code object
                ms.append(e0.elapsed_time(e1))
    emit(dict(kernels=True, tag=a.tag, pixels=P, columns=8, cameras=4, reps=a.kernel_reps,
              scoring_kernel_ms_median=float(np.median(ms)), scoring_kernel_ms_min=float(min(ms)),
              scoring_kernel_ms_max=float(max(ms)), timing="device events around one launch"))

    # the curve of a 16-weight ladder on the same frame (64 columns; printed, not asserted)
    r = solve_holdout(solver, G[0], f, K, betas=ladder16, camera_pixels=cams)
    emit(dict(curve=True, tag=a.tag, betas=ladder16.tolist(), cv_error=r.scores.cv_error.tolist(),
              cv_relative=r.scores.cv_relative.tolist(), train_error=r.scores.train_error.tolist(),
              selected=int(r.scores.selected), found=bool(r.scores.found)))


if __name__ == "__main__":
    main()
