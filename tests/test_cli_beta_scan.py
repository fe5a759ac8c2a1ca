"""sartsolver --beta_scan end to end on the fixture of test_cli_gpu_matches_gpu_semantics (two cameras, one stored
sparse, a Laplacian, four frames with saturated pixels): every dataset of /beta_scan, every column against the fp64
oracle at its own weight, the residual and roughness norms against NumPy on the stored values, the corner against the
rule's restatement on the file's own norms, /solution against the selected columns; on one rank and on two ranks sharing
the GPU."""
import os

import numpy as np
import pytest

import fit_bound
import rough_bound
from fp32_bound import fp32_errors
from mpi_cuda_sartsolver_amd.io.fixtures import make_case
from mpi_cuda_sartsolver_amd.ops import native
from test_cli_e2e import CLI_FP32_FACTOR, _frames, _laplacian
from test_lcurve_corner import corner_reference
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

pytestmark = pytest.mark.gpu

BETAS = (0.0, 1e-4, 1e-3, 1e-2, 1e-1)
SCAN = ["--beta_scan", "0,1e-4,1e-3,1e-2,1e-1", "-m", "60", "-c", "1e-6"]
T, NB, NVOXEL = 4, len(BETAS), 2048
FALLBACK = 3  # -b keeps its default 0.02: the nearest ladder entry is 1e-2
TYPES = {"beta": "<f8", "value": "<f8", "status": "<i4", "iterations": "<i4", "residual_norm": "<f8",
         "roughness_norm": "<f8", "curvature": "<f8", "selected": "<i4", "corner_found": "|u1"}


def _case(tmp_path):
    return make_case(str(tmp_path / "c"), sparse_cameras=("cam_b",), laplacian=True, nframes=T, saturate=0.05,
                     nvoxel=NVOXEL, grid=(16, 16, 16), shapes=((24, 32), (20, 30)))


def _read(path):
    n = native()
    d = {k: n.read_dataset_f64(path, "beta_scan/" + k) for k in TYPES}
    for k in ("value", "status", "iterations", "time"):
        d["solution/" + k] = n.read_dataset_f64(path, "solution/" + k)
    return d


_oracle_cache = {}


def _oracle_status(case, frames, L, log, k, i):
    """The tolerance-stopped oracle's status of frame k at weight i (the fixture is the same for every test)."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics

    key = ("status", log, k, i)
    if key not in _oracle_cache:
        _oracle_cache[key] = sart_gpu_semantics(case.A, frames[k], L, logarithmic=log, max_iterations=60,
                                                conv_tolerance=1e-6, beta_laplace=BETAS[i])[1]
    return _oracle_cache[key]


def check_columns(case, d, log, what):
    """Check 2: every column against the oracle run for the column's own recorded update count, at the fp32 bound."""
    frames, L = _frames(case), _laplacian(case)
    for k in range(T):
        for i in range(NB):
            e, e32 = fp32_errors(d["value"][k, i], case.A, frames[k], L, log=log, iterations=int(d["iterations"][k, i]),
                                 beta_laplace=BETAS[i])
            print(f"{what} frame {k} beta {BETAS[i]:g}: {int(d['iterations'][k, i])} updates, rel {e:.3e} "
                  f"fp32 emulation {e32:.3e}")
            assert e <= CLI_FP32_FACTOR * e32 + 1e-6, (k, i, e, e32)


def check_status(case, d, log):
    """Check 3."""
    frames, L = _frames(case), _laplacian(case)
    ref = np.array([[_oracle_status(case, frames, L, log, k, i) for i in range(NB)] for k in range(T)])
    np.testing.assert_array_equal(d["status"].astype(int), ref)


def check_norms(case, d, log, what):
    """Checks 4 and 5: the norms against NumPy on the stored values, at the fit and roughness bounds."""
    frames, L = _frames(case), _laplacian(case)
    P = case.A.shape[0]
    ell = np.asarray(case.A, dtype=np.float64).sum(axis=1)
    for k in range(T):
        F_ref, bound = fit_bound.reference(case.A, d["value"][k])
        eta2_ref, ebound = rough_bound.reference(L.row_ptr_host, L.col_host, L.val_host, d["value"][k], log)
        for i in range(NB):
            ref = fit_bound.stats_reference(F_ref[i], frames[k], ell, 1e-6, [P])
            tol = np.linalg.norm(np.where(ref["S"], bound[i], 0.0)) + 4 * P * fit_bound.U * ref["residual_norm"]
            rho, eta = d["residual_norm"][k, i], d["roughness_norm"][k, i]
            print(f"{what} frame {k} beta {BETAS[i]:g}: rho {rho:.17g} ref {ref['residual_norm']:.17g} tol {tol:.3e}; "
                  f"eta^2 {eta * eta:.17g} ref {eta2_ref[i]:.17g} bound {ebound[i]:.3e}")
            assert abs(rho - ref["residual_norm"]) <= tol, (k, i)
            # the file holds sqrt(eta2): the root and this square add three roundings of eta2
            assert abs(eta * eta - eta2_ref[i]) <= ebound[i] + 4 * rough_bound.U * eta2_ref[i], (k, i)


def check_corner_and_solution(d):
    """Checks 6 and 7: the corner rule on the file's own norms, and /solution against the selected columns."""
    for k in range(T):
        sel, found, curv = corner_reference(d["residual_norm"][k], d["roughness_norm"][k], np.ones(NB, dtype=np.uint8),
                                            FALLBACK)
        assert int(d["selected"][k]) == sel and bool(d["corner_found"][k]) == found, k
        assert np.array_equal(d["curvature"][k], curv, equal_nan=True), k
        assert np.array_equal(d["solution/value"][k], d["value"][k, sel]), k
        assert int(d["solution/status"][k]) == int(d["status"][k, sel])
        assert int(d["solution/iterations"][k]) == int(d["iterations"][k, sel])
    print("selected", d["selected"], "found", d["corner_found"])


def _run(tmp_path, binary, case, log, name, nproc=1):  # noqa: F811
    out = str(tmp_path / name)
    argv = SCAN + ["-l", case.laplacian_file, "-o", out] + (["-L"] if log else []) + case.files
    r = _run_native(binary, argv, nproc=nproc)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out, r


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
def test_cli_beta_scan(tmp_path, binary, log):  # noqa: F811
    case = _case(tmp_path)
    out, r = _run(tmp_path, binary, case, log, "scan.h5")
    assert r.stdout.count("Processed in:") == T, r.stdout
    assert f"Beta scan of {T} frame(s) x {NB} weights in:" in r.stdout
    n = native()
    d = _read(out)
    # check 1: shapes and stored types
    shapes = {"beta": (NB,), "value": (T, NB, NVOXEL), "selected": (T,), "corner_found": (T,)}
    for name, dtype in TYPES.items():
        assert d[name].shape == shapes.get(name, (T, NB)), name
        assert n.dataset_dtype(out, "beta_scan/" + name) == dtype, name
    np.testing.assert_array_equal(d["beta"], BETAS)
    assert d["solution/value"].shape == (T, NVOXEL)
    np.testing.assert_allclose(d["solution/time"], next(iter(case.times.values())), atol=1e-12)
    assert n.read_dataset_f64(out, "voxel_map/i").size > 0  # the voxel map is copied as in any run
    assert np.all(np.isfinite(d["value"])) and np.all(d["iterations"] >= 1) and np.all(d["iterations"] <= 60)
    check_columns(case, d, log, "one rank")
    check_status(case, d, log)
    check_norms(case, d, log, "one rank")
    check_corner_and_solution(d)
    # the weights matter: a frame's columns differ, and a heavier weight gives a smoother solution
    assert np.all(d["roughness_norm"][:, -1] < d["roughness_norm"][:, 0])


def test_cli_beta_scan_two_ranks_one_device(tmp_path, binary):  # noqa: F811
    """Two ranks on one GPU (staged reductions over TCP, as test_cli_fp64_two_ranks_one_device launches). Solutions of
    different pixel partitions differ at fp32 level: the fp32 bound is the criterion, and the residual norms stay
    within 1e-4 relative of the one-rank file's."""
    case = _case(tmp_path)
    one, _ = _run(tmp_path, binary, case, False, "one.h5")
    saved = {k: os.environ.get(k) for k in ("SART_DIST_BACKEND", "SART_P2P")}
    os.environ["SART_DIST_BACKEND"] = "tcp"
    os.environ["SART_P2P"] = "0"
    try:
        two, r = _run(tmp_path, binary, case, False, "two.h5", nproc=2)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert r.stdout.count("Processed in:") == T, r.stdout
    d, d1 = _read(two), _read(one)
    check_columns(case, d, False, "two ranks")
    check_norms(case, d, False, "two ranks")
    check_corner_and_solution(d)
    rel = np.abs(d["residual_norm"] - d1["residual_norm"]) / d1["residual_norm"]
    print(f"residual_norm, two ranks against one: max relative difference {rel.max():.3e}")
    assert np.all(rel <= 1e-4)
