#!/usr/bin/env python3
"""Phantoms against a batch of distinct frames, one session, on the ray-traced 64k x 64k matrix of the storage
benchmarks (tools/storage_bench.py), cold 20-update solves:

* (a) 16 phantoms through ``models.phantom.solve_phantoms``: the fp64 projections of the truths (``fit_forward``, two
  passes of 8), ``MultiFrameSARTSolver(batch=16).solve_batch`` of the 16 columns, then the scoring kernel and the
  scores of every column;
* (b) ``solve_batch`` of 16 distinct ordinary frames on the same solver: the same kernels and bytes, only the source of
  the frames and one small pass per phantom differ.

The cases alternate within the session (``--repeats`` rounds of ``--reps`` timed solves each after ``--warmup`` untimed
ones); the spread of a case's rounds is the run-to-run spread a difference has to exceed. JSON lines; the summary line
carries the ratio a/b of the column-iterations per second (expected >= 0.85). A last line times the projection kernel
(8 truths per pass) and the scoring kernel (8 columns per pass) alone: device events around one launch, median of
``--kernel-reps``.

    python tools/phantom_bench.py --out profiles/phantom_64k.jsonl
    python tools/phantom_bench.py --nvox 4096 --cam 32x32 --reps 2          # a small shape

Host clock around calls that return host arrays (i.e. end synchronised). Not measured: multi-GPU runs, other batch
widths, other storages, replicas of phantoms, the native driver's read-ahead overlap of the projection with the solve,
hardware counters (PMC).
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
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from mpi_cuda_sartsolver_amd.models.fit import fit_forward_device
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.phantom import solve_phantoms
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams
    from mpi_cuda_sartsolver_amd.ops import hip
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
    NC = 16
    t0 = time.perf_counter()
    cam = tuple(int(v) for v in a.cam.split("x"))
    A, X, _, grid, _, rng = parity.raytraced_problem(a.nvox, cam, nframes=NC)
    rtm = DenseRTM.from_dense(A, device=dev)
    G = parity.frames_from(rtm.A[: rtm.npixel, : rtm.nvoxel], X, rng)
    P, V = A.shape
    del A
    truths = np.abs(np.asarray(X, dtype=np.float64))[:NC]  # the phantoms the frames of (b) were made from
    solver = MultiFrameSARTSolver(rtm, None, None, SolverParams(beta_laplace=0.0, max_iterations=a.steps,
                                                                conv_tolerance=0.0),
                                  batch=NC, allow_zero_tolerance=True)

    run = {"a": lambda: solve_phantoms(solver, truths)[0].columns, "b": lambda: solver.solve_batch(G[:NC])}
    cases = ["a", "b"]
    emit(dict(setup=True, tag=a.tag, shape=[P, V], grid=list(grid), steps=a.steps, warmup=a.warmup, reps=a.reps,
              repeats=a.repeats, columns=NC, phantoms=NC, seconds=time.perf_counter() - t0,
              device=torch.cuda.get_device_name(dev), forward_split=solver.forward_split,
              timing="host clock around calls that return host arrays; cases alternate within the session",
              not_measured="multi-GPU runs, other batch widths and storages, replicas of phantoms, the native driver's "
                           "read-ahead overlap, hardware counters (PMC)"))
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

    # the two kernels alone
    k = hip()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        Xd = torch.zeros((8, rtm.ld), dtype=torch.float64, device=dev)
        Xd[:, :V] = torch.from_numpy(truths[:8]).to(dev)
        Fd = torch.zeros((8, rtm.nrows_pad), dtype=torch.float64, device=dev)
        td = torch.from_numpy(truths[8]).to(dev)
        sums = torch.empty((8, 10), dtype=torch.float64, device=dev)
        scratch = torch.empty(int(k.phantom64_scratch_elems(V)), dtype=torch.float64, device=dev)
        launches = {
            "projection": lambda: fit_forward_device(rtm, Xd, 8, Fd, stream=stream.cuda_stream),
            "scoring": lambda: k.phantom64(Xd.data_ptr(), rtm.ld, V, 8, td.data_ptr(), sums.data_ptr(),
                                           scratch.data_ptr(), stream.cuda_stream),
        }
        ms = {name: [] for name in launches}
        for name, launch in launches.items():
            for i in range(a.kernel_reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if i:  # the first launch loads the code object
                    ms[name].append(e0.elapsed_time(e1))
    emit(dict(kernels=True, tag=a.tag, shape=[P, V], vectors_per_pass=8, reps=a.kernel_reps,
              projection_kernel_ms_median=float(np.median(ms["projection"])),
              projection_kernel_ms_min=float(min(ms["projection"])), projection_kernel_ms_max=float(max(ms["projection"])),
              scoring_kernel_ms_median=float(np.median(ms["scoring"])), scoring_kernel_ms_min=float(min(ms["scoring"])),
              scoring_kernel_ms_max=float(max(ms["scoring"])),
              timing="device events around one launch (the scoring: both of its kernels)"))


if __name__ == "__main__":
    main()
