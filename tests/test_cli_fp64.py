"""sartsolver --fp64 end to end on the dense fixture case of tests/test_cli_e2e.py and tests/test_native_driver.py (two
cameras, one of them stored sparse, a Laplacian, several frames with saturated pixels): --fp64_semantics cpu against
the --use_cpu file, on one rank and on two ranks sharing the GPU; --fp64 (gpu semantics) against
CPUSARTSolver(semantics="gpu") chained over the frames; the --profile load line."""
import json
import os

import numpy as np
import pytest

from mpi_cuda_sartsolver_amd.io.fixtures import make_case
from mpi_cuda_sartsolver_amd.ops import native
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

pytestmark = pytest.mark.gpu


def _case(tmp_path):
    return make_case(str(tmp_path / "case"), sparse_cameras=("cam_b",), laplacian=True, nframes=3, saturate=0.05)


def _read(path):
    n = native()
    d = {k: n.read_dataset_f64(path, "solution/" + k) for k in ("value", "status", "iterations", "time")}
    d["value"] = d["value"].reshape(d["time"].size, -1)
    return d


def _same(a, b):
    """status, iterations and time equal; every frame's solution within 1e-9 of its maximum"""
    for k in ("status", "iterations", "time"):
        np.testing.assert_array_equal(a[k], b[k])
    for xa, xb in zip(a["value"], b["value"]):
        e = np.max(np.abs(xa - xb)) / np.max(np.abs(xb))
        print(f"max|x - x_ref| / max|x_ref| = {e:.3e}")
        assert e <= 1e-9


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
def test_cli_fp64_cpu_semantics_equals_use_cpu(tmp_path, binary, log):  # noqa: F811
    case = _case(tmp_path)
    base = ["-m", "80", "-c", "1e-7", "-l", case.laplacian_file, "-b", "1e-3"] + (["-L"] if log else [])
    cpu, gpu, prof = str(tmp_path / "cpu.h5"), str(tmp_path / "gpu.h5"), str(tmp_path / "p.jsonl")
    r = _run_native(binary, base + ["--use_cpu", "-o", cpu, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run_native(binary, base + ["--fp64", "--fp64_semantics", "cpu", "--profile", prof, "-o", gpu, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("Processed in:") == 3 and "sparse: " not in r.stdout  # auto loads the shard dense
    _same(_read(gpu), _read(cpu))
    recs = [json.loads(line) for line in open(prof)]
    load = recs[0]
    assert load["load"] and load["solver_path"] == "fp64-two-pass" and load["fp64_semantics"] == "cpu", load
    assert load["rtm_format"] == "dense" and load["rtm_storage"] == "fp32"
    assert len(recs) == 4 and all(rec["fused"] is False for rec in recs[1:])


def test_cli_fp64_two_ranks_one_device(tmp_path, binary):  # noqa: F811
    """Two ranks on one GPU (staged reductions over TCP, as test_native_sparse_two_ranks_one_device launches) against
    the one-rank --use_cpu file."""
    case = _case(tmp_path)
    base = ["-m", "80", "-c", "1e-7", "-l", case.laplacian_file, "-b", "1e-3"]
    cpu, two = str(tmp_path / "cpu.h5"), str(tmp_path / "two.h5")
    r = _run_native(binary, base + ["--use_cpu", "-o", cpu, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    saved = {k: os.environ.get(k) for k in ("SART_DIST_BACKEND", "SART_P2P")}
    os.environ["SART_DIST_BACKEND"] = "tcp"
    os.environ["SART_P2P"] = "0"
    try:
        r = _run_native(binary, base + ["--fp64", "--fp64_semantics", "cpu", "-o", two, *case.files], nproc=2)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    _same(_read(two), _read(cpu))


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
def test_cli_fp64_gpu_semantics_equals_cpu_solver(tmp_path, binary, log):  # noqa: F811
    """--fp64 with the default semantics: CPUSARTSolver(semantics="gpu") on the case's matrices, warm-started frame
    to frame as the driver does."""
    from mpi_cuda_sartsolver_amd.models.cpu import CPUSARTSolver
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams
    from test_cli_e2e import _frames, _laplacian

    case = _case(tmp_path)
    out, prof = str(tmp_path / "gpu.h5"), str(tmp_path / "p.jsonl")
    argv = ["-m", "80", "-c", "1e-7", "-l", case.laplacian_file, "-b", "1e-3", "--fp64", "--profile", prof, "-o", out]
    r = _run_native(binary, argv + (["-L"] if log else []) + case.files)
    assert r.returncode == 0, r.stdout + r.stderr
    s = CPUSARTSolver(case.A, _laplacian(case), params=SolverParams(max_iterations=80, conv_tolerance=1e-7,
                                                                   beta_laplace=1e-3), logarithmic=log, semantics="gpu")
    got, prev = _read(out), None
    for k, g in enumerate(_frames(case)):
        ref = s.solve(g, solution=prev)
        prev = ref.solution
        assert (int(got["status"][k]), int(got["iterations"][k])) == (ref.status, ref.iterations)
        e = np.max(np.abs(got["value"][k] - ref.solution)) / np.max(np.abs(ref.solution))
        print(f"frame {k}: max|x - x_ref| / max|x_ref| = {e:.3e}")
        assert e <= 1e-9
    load = json.loads(open(prof).readline())
    assert load["solver_path"] == "fp64-two-pass" and load["fp64_semantics"] == "gpu", load
