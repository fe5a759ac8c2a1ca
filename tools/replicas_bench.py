#!/usr/bin/env python3
"""Replicas of one frame against a batch of distinct frames, one session, on the ray-traced 64k x 64k matrix of the
storage benchmarks (tools/storage_bench.py), cold 20-update solves:

* (a) the nominal frame and 15 noisy replicas of it: ``perturbed_frames`` (the noise kernel and its copies) and
  ``MultiFrameSARTSolver(batch=16).solve_batch`` of the 16 columns, then ``replica_moments`` -- what
  ``models.uncertainty.solve_replicas`` runs;
* (b) ``solve_batch`` of 16 distinct frames on the same solver: the same kernels and bytes, only the source of the
  frames differs.

The cases alternate within the session (``--repeats`` rounds of ``--reps`` timed solves each after ``--warmup`` untimed
ones); the spread of a case's rounds is the run-to-run spread a difference has to exceed. JSON lines; the summary line
carries the ratio a/b of the column-iterations per second (expected >= 0.85). A last line times the noise kernel for 64
replicas of 65536 pixels (device events around the launch, median of ``--noise-reps``) against the NumPy emulation
(utils/philox.py::perturb) of the same on the host.

    python tools/replicas_bench.py --out profiles/replicas_64k.jsonl
    python tools/replicas_bench.py --nvox 4096 --cam 32x32 --reps 2          # a small shape

Host clock around calls that return host arrays (i.e. end synchronised). Not measured: multi-GPU runs, other batch
widths, other storages, the native driver's read-ahead overlap, hardware counters (PMC).
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
    ap.add_argument("--noise-pixels", type=int, default=65536)
    ap.add_argument("--noise-replicas", type=int, default=64)
    ap.add_argument("--noise-reps", type=int, default=9)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams
    from mpi_cuda_sartsolver_amd.models.uncertainty import perturbed_frames, replica_moments
    from mpi_cuda_sartsolver_amd.ops import hip
    from mpi_cuda_sartsolver_amd.utils import parity, philox

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
    NC, NREP, TIME, SEED, REL = 16, 15, 0.125, 1, 0.02
    t0 = time.perf_counter()
    cam = tuple(int(v) for v in a.cam.split("x"))
    A, X, _, grid, _, rng = parity.raytraced_problem(a.nvox, cam, nframes=NC)
    rtm = DenseRTM.from_dense(A, device=dev)
    G = parity.frames_from(rtm.A[: rtm.npixel, : rtm.nvoxel], X, rng)
    P, V = A.shape
    del A
    noise = dict(abs=1e-3 * float(G[0].max()), shot=0.0, rel=REL)
    solver = MultiFrameSARTSolver(rtm, None, None, SolverParams(beta_laplace=0.0, max_iterations=a.steps,
                                                                conv_tolerance=0.0),
                                  batch=NC, allow_zero_tolerance=True)
    part = {"noise_s": [], "solve_s": [], "moments_s": []}

    def replicas():
        t = time.perf_counter()
        frames = perturbed_frames(G[0], TIME, NREP, seed=SEED, device=dev, **noise)
        t1 = time.perf_counter()
        cols = solver.solve_batch(frames)
        t2 = time.perf_counter()
        replica_moments(np.stack([r.solution for r in cols[1:]]), device=dev)
        t3 = time.perf_counter()
        part["noise_s"].append(t1 - t), part["solve_s"].append(t2 - t1), part["moments_s"].append(t3 - t2)
        return cols

    run = {"a": replicas, "b": lambda: solver.solve_batch(G[:NC])}
    cases = ["a", "b"]
    emit(dict(setup=True, tag=a.tag, shape=[P, V], grid=list(grid), steps=a.steps, warmup=a.warmup, reps=a.reps,
              repeats=a.repeats, columns=NC, replicas=NREP, noise=noise, seconds=time.perf_counter() - t0,
              device=torch.cuda.get_device_name(dev), forward_split=solver.forward_split,
              timing="host clock around calls that return host arrays; cases alternate within the session",
              not_measured="multi-GPU runs, other batch widths and storages, the native driver's read-ahead overlap, "
                           "hardware counters (PMC)"))
    for c in cases:
        for _ in range(a.warmup):
            run[c]()
    for v in part.values():
        v.clear()
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
              a_parts_ms_median={k: 1e3 * float(np.median(v)) for k, v in part.items()},
              a_over_b=med["b"] / med["a"], expected_at_least=0.85))  # rates: (a) / (b)

    # the noise kernel alone against the NumPy emulation
    n, nrep = a.noise_pixels, a.noise_replicas
    g = np.abs(np.random.default_rng(0).standard_normal(n)) + 0.1
    k = hip()
    ldo = (n + 63) // 64 * 64
    with torch.cuda.device(dev):
        gd = torch.from_numpy(g).to(dev)
        buf = torch.empty((nrep, ldo), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev)
        ms = []
        for i in range(a.noise_reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            k.noise_replicas(gd.data_ptr(), n, 0, philox.time_bits(TIME), 1, nrep, 0.05, 0.01, REL, SEED,
                             buf.data_ptr(), ldo, stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            if i:  # the first launch loads the code object
                ms.append(e0.elapsed_time(e1))
        dev_out = buf[:, :n].cpu().numpy()
    t = time.perf_counter()
    ref = philox.perturb(g, TIME, nrep, 0.05, 0.01, REL, SEED)
    host_s = time.perf_counter() - t
    emit(dict(noise_kernel=True, tag=a.tag, pixels=n, replicas=nrep, kernel_ms_median=float(np.median(ms)),
              kernel_ms_min=float(min(ms)), kernel_ms_max=float(max(ms)), reps=a.noise_reps,
              numpy_emulation_ms=1e3 * host_s, host_cpus=os.cpu_count(),
              normals_per_s_kernel=n * nrep / (1e-3 * float(np.median(ms))),
              max_abs_difference=float(np.abs(dev_out - ref[1:]).max()),
              timing="device events around one launch; the emulation: host clock around perturb(), single thread"))


if __name__ == "__main__":
    main()
