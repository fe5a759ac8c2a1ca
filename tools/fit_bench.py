#!/usr/bin/env python3
"""The fit kernels (csrc/kernels/fit64.hip) at size, one session, device events: per storage one pass over the shard
with nv = 1, 4 and 8 solutions, against the yardstick of the same bytes and FMAs -- k_forward64 (projection64.hip) on
the fp32 shard at nv = 1 -- and whether grouping pays (one nv = 8 pass against eight nv = 1 passes). Cases alternate
within the session (round-robin over ``--passes`` rounds after ``--warmup`` rounds); JSON lines, with a summary line
and a README table row.

    python tools/fit_bench.py --out profiles/fit_64k.jsonl
    python tools/fit_bench.py --pixels 4096 --voxels 8192 --no-sparse     # a small shape

Dense: ``DenseRTM.synthetic`` (fp32, and its bf16 and row-scaled f16 copies). Sparse: the ray-traced direct matrix of
tools/sparse_bench.py (two cameras of 128 x 256 pixels on a 32 x 32 x 64 grid at the default size).
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
    ap.add_argument("--pixels", type=int, default=65536)
    ap.add_argument("--voxels", type=int, default=65536)
    ap.add_argument("--passes", type=int, default=20, help="timed passes per case")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sparse", action="store_true")
    ap.add_argument("--sparse-grid", default="32,32,64")
    ap.add_argument("--sparse-shape", default="128,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from mpi_cuda_sartsolver_amd.models.fit import fit_forward_device
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM, SparseRTM
    from mpi_cuda_sartsolver_amd.ops import hip

    k = hip()
    dev = torch.device("cuda", 0)
    outf = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()

    t0 = time.perf_counter()
    P, V = a.pixels, a.voxels
    shards = {"fp32": DenseRTM.synthetic(P, V, device=dev)}
    shards["bf16"] = shards["fp32"].to_bf16()
    shards["f16"] = shards["fp32"].to_f16()
    if not a.no_sparse:
        from mpi_cuda_sartsolver_amd.utils.raytrace import Camera, default_cameras, raytraced_direct_coo

        grid = tuple(int(x) for x in a.sparse_grid.split(","))
        H, W = (int(x) for x in a.sparse_shape.split(","))
        cams = [Camera(f"cam_{i}", b.position, b.look_at, (H, W), b.field_of_view, b.up)
                for i, b in enumerate(default_cameras(n=2))]
        r, c, v, _ = raytraced_direct_coo(grid=grid, cameras=cams)
        shards["sparse"] = SparseRTM.from_entries(2 * H * W, int(np.prod(grid)), r, c, v, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(0)
    cases, bytes_of = {}, {}
    for name, m in shards.items():
        sparse = name == "sparse"
        X = torch.zeros((8, m.ld), dtype=torch.float64, device=dev)
        X[:, : m.nvoxel] = torch.from_numpy(rng.random((8, m.nvoxel)))
        F = torch.zeros((8, m.nrows_pad), dtype=torch.float64, device=dev)
        Xt = torch.zeros((m.ld, 8), dtype=torch.float64, device=dev) if sparse else None
        # matrix bytes of one pass: the shard as stored; CSR: value + column index per entry and the row offsets
        bytes_of[name] = (m.nnz * 8 + (m.npixel + 1) * 8) if sparse else m.npixel * m.ld * m.A.element_size()
        for nv in (1, 4, 8):
            cases[(name, nv)] = (lambda m=m, X=X, F=F, Xt=Xt, nv=nv:
                                 fit_forward_device(m, X, nv, F, Xt=Xt, stream=stream))
        if name == "fp32":  # the yardstick: the fp64 engine's forward projection on the same shard
            x1 = X[0].contiguous()
            f1 = torch.zeros(m.nrows_pad, dtype=torch.float64, device=dev)
            cases[("forward64", 1)] = (lambda m=m, x1=x1, f1=f1:
                                       k.forward64(0, m.A.data_ptr(), m.ld, m.npixel, m.nrows_pad, m.nvoxel,
                                                   x1.data_ptr(), 0, 0, f1.data_ptr(), 0, 0, 0, stream))
            bytes_of["forward64"] = bytes_of["fp32"]
    torch.cuda.synchronize(dev)
    emit(dict(setup=True, shape=[P, V], passes=a.passes, warmup=a.warmup, seconds=time.perf_counter() - t0,
              device=torch.cuda.get_device_name(dev), sparse_shape=None if a.no_sparse else
              [shards["sparse"].npixel, shards["sparse"].nvoxel, shards["sparse"].nnz],
              timing="device events around each pass; cases round-robin within one session",
              not_measured="multi-GPU, other widths, hardware counters (PMC), the driver's end-to-end share"))
    ms = {c: [] for c in cases}
    for rnd in range(a.warmup + a.passes):
        for c, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= a.warmup:
                ms[c].append(e0.elapsed_time(e1))
    med = {c: float(np.median(v)) for c, v in ms.items()}
    for (name, nv), t in med.items():
        emit(dict(case=name, nv=nv, ms_median=t, ms_min=float(np.min(ms[(name, nv)])),
                  ms_max=float(np.max(ms[(name, nv)])), matrix_TBps=bytes_of[name] / (1e-3 * t) / 1e12,
                  frames_per_matrix_read=nv))
    summary = dict(summary=True, shape=[P, V],
                   fit_fp32_nv1_over_forward64=med[("forward64", 1)] / med[("fp32", 1)], expected_at_least=0.85)
    row = []
    for name in shards:
        ratio = 8 * med[(name, 1)] / med[(name, 8)]
        best = max((1, 4, 8), key=lambda nv: nv / med[(name, nv)])
        summary[name] = dict(eight_nv1_over_one_nv8=ratio, grouping_pays=bool(ratio > 1.0), best_nv=best,
                             ms_nv1=med[(name, 1)], ms_nv4=med[(name, 4)], ms_nv8=med[(name, 8)],
                             matrix_TBps_nv8=bytes_of[name] / (1e-3 * med[(name, 8)]) / 1e12)
        row.append(f"{name} {med[(name, 1)]:.2f} / {med[(name, 8)]:.2f} ms ({ratio:.1f}x)")
    emit(summary)
    print("| fit pass, nv = 1 / nv = 8 (8 x nv1 / nv8) | " + "; ".join(row) +
          f" | fp32 nv = 1 at {summary['fit_fp32_nv1_over_forward64']:.2f}x k_forward64 |")


if __name__ == "__main__":
    main()
