"""sartsolver --holdout end to end on the fixture of tests/test_cli_replicas.py (two cameras of 24 x 32 and 20 x 30
pixels of which the frame masks keep 602 and 487, one stored sparse, a Laplacian, 5 % saturated pixels, two frames):
`--holdout 4 --holdout_betas 0,1e-3,1e-2 -m 60 -c 1e-6`.

Check 1: the datasets of /holdout by name, stored type and shape; `folds` is the NumPy table, `beta` the ladder.
Check 2: every stored column against the fp64 oracle on the NumPy-masked frame for the column's recorded update count,
at the beta-scan column rule.
Check 3: `sums` against utils.holdout.sums_reference on `case.A.astype(float64) @ x` of the stored columns at 1e-9
relative. The kernel's images come from the fit kernels, whose fp64 sums over <= 2048 products differ from NumPy's in
their order alone: below 1e-12 of sum |a x| = f per pixel, so a sum of (g - f)^2 over a pixel set moves by at most
2 ||g - f|| 1e-12 ||f||, that is 2e-12 ||f|| / ||g - f|| of itself. The test asserts the precondition that the residual
norm of every (column, camera, set) is at least 1e-3 of its image norm and prints the smallest ratio.
Then: the derived datasets are bit for bit the native scores of the stored sums; /solution is column 0 of the selected
weight; SART_FIT_GROUP=1 writes the same /holdout; `--holdout cameras` without a ladder; two ranks sharing the GPU;
f16 and sparse storage with the --profile line.

Not tested: the driver's refusal of 2^32 pixels and more (no fixture of that size is practical)."""
import json
import os

import numpy as np
import pytest

from fp32_bound import fp32_errors
from mpi_cuda_sartsolver_amd.io.fixtures import make_case
from mpi_cuda_sartsolver_amd.ops import native
from mpi_cuda_sartsolver_amd.utils import holdout as ho
from test_cli_e2e import CLI_FP32_FACTOR, _frames, _laplacian
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

pytestmark = pytest.mark.gpu

T, K, NVOXEL, B = 2, 4, 2048, 1e-3
BETAS = [0.0, 1e-3, 1e-2]
CAMS = (602, 487)  # the pixels the fixture's frame masks keep, per camera in composite order (_case asserts them)
NPIXEL = sum(CAMS)
THR = 1e-6  # -r's default
TYPES = {"folds": "<i4", "seed": "<u8", "beta": "<f8", "value": "<f8", "status": "<i4", "iterations": "<i4",
         "sums": "<f8", "cv_error": "<f8", "cv_relative": "<f8", "train_error": "<f8", "cv_error_camera": "<f8",
         "eligible": "|u1", "selected": "<i4", "found": "|u1"}
DERIVED = ("cv_error", "cv_relative", "train_error", "cv_error_camera", "eligible")


def _case(tmp_path):
    case = make_case(str(tmp_path / "c"), sparse_cameras=("cam_b",), laplacian=True, nframes=T, saturate=0.05,
                     nvoxel=NVOXEL, grid=(16, 16, 16), shapes=((24, 32), (20, 30)))
    assert tuple(int((case.masks[c] > 0).sum()) for c in sorted(case.masks)) == CAMS and case.npixel == NPIXEL
    return case


def _run(tmp_path, binary, case, name, mode=("--holdout", str(K), "--holdout_betas", "0,1e-3,1e-2"), extra=(),  # noqa: F811
         nproc=1, env=None):
    out = str(tmp_path / name)
    argv = [*mode, "-m", "60", "-c", "1e-6", "-l", case.laplacian_file, "-b", repr(B), *extra, "-o", out, *case.files]
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        res = _run_native(binary, argv, nproc=nproc)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count("Processed in:") == T, res.stdout
    assert "Hold-out of 2 frame(s) x " in res.stdout
    return out


def _read(path):
    n = native()
    d = {k: n.read_dataset_f64(path, "holdout/" + k) for k in TYPES}
    d["mode"] = n.read_dataset_string(path, "holdout/mode")
    for k in ("value", "status", "iterations", "time"):
        d["solution/" + k] = n.read_dataset_f64(path, "solution/" + k)
    return d


def check_columns(case, d, folds, betas, what):
    """Check 2."""
    L, G = _laplacian(case), _frames(case)
    nc = int(folds.max()) + 2
    for k in range(T):
        M = ho.masked_frames(G[k], folds, nc - 1)
        for i, beta in enumerate(betas):
            for c in range(nc):
                it = int(d["iterations"][k, i, c])
                e, e32 = fp32_errors(d["value"][k, i, c], case.A, M[c], L, iterations=it, beta_laplace=beta)
                print(f"{what} frame {k} beta {beta:g} column {c}: {it} updates, rel {e:.3e} fp32 emulation {e32:.3e}")
                assert e <= CLI_FP32_FACTOR * e32 + 1e-6, (k, i, c, e, e32)


def check_sums(case, d, folds, what):
    """Check 3, with its precondition."""
    A64, G = case.A.astype(np.float64), _frames(case)
    ell = A64 @ np.ones(NVOXEL)
    nb, nc = d["value"].shape[1:3]
    held = np.tile(np.arange(-1, nc - 1, dtype=np.int32), nb)
    starts = np.concatenate([[0], np.cumsum(CAMS)])
    worst = np.inf
    for k in range(T):
        F = d["value"][k].reshape(nb * nc, NVOXEL) @ A64.T
        want = ho.sums_reference(F, G[k], ell, THR, folds, held, CAMS).reshape(nb, nc, len(CAMS), 6)
        got = d["sums"][k]
        assert np.array_equal(got[..., [2, 5]], want[..., [2, 5]]), (what, k)  # the counts are exact
        valid = (G[k] >= 0) & (ell > THR)
        for j in range(nb * nc):
            for m in range(len(CAMS)):
                cam = np.zeros(NPIXEL, dtype=bool)
                cam[starts[m]: starts[m + 1]] = True
                hold = valid & cam & (folds == held[j])
                for q, S in ((0, hold), (3, valid & cam & ~hold)):
                    if S.any():
                        ratio = np.sqrt(want.reshape(nb * nc, len(CAMS), 6)[j, m, q]) / np.linalg.norm(F[j, S])
                        worst = min(worst, ratio)
        err = np.abs(got - want) / np.where(want > 0, want, 1.0)
        print(f"{what} frame {k}: sums max relative difference {err.max():.3e}")
        assert err.max() <= 1e-9, (what, k, err.max())
    print(f"{what}: smallest residual norm / image norm over (column, camera, set) = {worst:.3e}")
    assert worst >= 1e-3, worst


def check_scores_and_solution(d, fallback, what):
    n = native()
    nb, nc = d["value"].shape[1:3]
    for k in range(T):
        cv, rel, train, cam, elig, sel, found = n.holdout_scores(d["sums"][k], np.ones((nb, nc), dtype=np.uint8), fallback)
        want = dict(zip(DERIVED, (cv, rel, train, cam, elig)))
        for name in DERIVED:
            assert np.array_equal(d[name][k], np.asarray(want[name], dtype=np.float64), equal_nan=True), (what, k, name)
        assert int(d["selected"][k]) == sel and int(d["found"][k]) == found == 1, (what, k)
        assert sel == int(np.argmin(cv))
        assert np.array_equal(d["solution/value"][k], d["value"][k, sel, 0]), (what, k)
        assert int(d["solution/status"][k]) == int(d["status"][k, sel, 0])
        assert int(d["solution/iterations"][k]) == int(d["iterations"][k, sel, 0])
        print(f"{what} frame {k}: cv_error {cv} train_error {train} selected {sel}")


def test_cli_holdout(tmp_path, binary):  # noqa: F811
    case = _case(tmp_path)
    out = _run(tmp_path, binary, case, "ho.h5")
    n = native()
    d = _read(out)
    # check 1
    nb, nc, ncam = len(BETAS), K + 1, len(CAMS)
    shapes = {"folds": (NPIXEL,), "seed": (1,), "beta": (nb,), "value": (T, nb, nc, NVOXEL), "status": (T, nb, nc),
              "iterations": (T, nb, nc), "sums": (T, nb, nc, ncam, 6), "cv_error": (T, nb), "cv_relative": (T, nb),
              "train_error": (T, nb), "cv_error_camera": (T, nb, ncam), "eligible": (T, nb), "selected": (T,),
              "found": (T,)}
    for name, dtype in TYPES.items():
        assert n.dataset_dtype(out, "holdout/" + name) == dtype, name
        assert d[name].shape == shapes[name], name
    assert d["mode"] == "pixels" and int(d["seed"][0]) == 0
    folds = ho.folds(NPIXEL, K, 0)
    assert np.array_equal(d["folds"], folds)
    np.testing.assert_array_equal(d["beta"], BETAS)
    assert d["solution/value"].shape == (T, NVOXEL)
    np.testing.assert_allclose(d["solution/time"], np.asarray(next(iter(case.times.values()))), atol=1e-12)
    assert n.read_dataset_f64(out, "voxel_map/i").size > 0  # the voxel map is copied as in any run
    assert np.all(np.isfinite(d["value"])) and np.all(d["iterations"] >= 1) and np.all(d["iterations"] <= 60)
    assert np.all(d["eligible"] == 1)
    check_columns(case, d, folds, BETAS, "one rank")
    check_sums(case, d, folds, "one rank")
    check_scores_and_solution(d, 1, "one rank")  # -b 1e-3 names entry 1
    # the projection groups do not show in the file
    d1 = _read(_run(tmp_path, binary, case, "g1.h5", env={"SART_FIT_GROUP": "1"}))
    assert d1["mode"] == d["mode"]
    for name in (*TYPES, "solution/value"):
        assert np.array_equal(d1[name], d[name], equal_nan=True), name


def test_cli_holdout_cameras(tmp_path, binary):  # noqa: F811
    """Leave one camera out, at -b alone: K = 2, the fold is the camera, cv_error_camera[m] is column m + 1's."""
    case = _case(tmp_path)
    d = _read(_run(tmp_path, binary, case, "cam.h5", mode=("--holdout", "cameras")))
    folds = np.repeat(np.arange(2, dtype=np.int32), CAMS)
    assert d["mode"] == "cameras" and np.array_equal(d["folds"], folds) and int(d["seed"][0]) == 0
    np.testing.assert_array_equal(d["beta"], [B])
    assert d["value"].shape == (T, 1, 3, NVOXEL) and d["sums"].shape == (T, 1, 3, 2, 6)
    check_columns(case, d, folds, [B], "cameras")
    check_sums(case, d, folds, "cameras")
    check_scores_and_solution(d, 0, "cameras")
    s = d["sums"][:, 0]
    assert np.all(s[:, 1, 1, :3] == 0) and np.all(s[:, 2, 0, :3] == 0) and np.all(s[:, 1, 0, 3:] == 0)
    for m in range(2):
        assert np.array_equal(d["cv_error_camera"][:, 0, m], np.sqrt(s[:, m + 1, m, 0] / s[:, m + 1, m, 2]))


def test_cli_holdout_cameras_needs_two(tmp_path, binary):  # noqa: F811
    case = make_case(str(tmp_path / "one"), cameras=("cam_a",), shapes=((6, 8),), nframes=1)
    res = _run_native(binary, ["--holdout", "cameras", "-o", str(tmp_path / "x.h5"), *case.files])
    assert res.returncode != 0
    assert "Argument holdout cameras needs at least two cameras, 1 given." in res.stderr


def test_cli_holdout_two_ranks_one_device(tmp_path, binary):  # noqa: F811
    """Two ranks on one GPU (the environment of test_cli_replicas_two_ranks_one_device): the second rank masks its
    pixels by their global indices."""
    case = _case(tmp_path)
    d = _read(_run(tmp_path, binary, case, "two.h5", nproc=2, env={"SART_DIST_BACKEND": "tcp", "SART_P2P": "0"}))
    folds = ho.folds(NPIXEL, K, 0)
    assert np.array_equal(d["folds"], folds)
    check_columns(case, d, folds, BETAS, "two ranks")
    check_sums(case, d, folds, "two ranks")
    check_scores_and_solution(d, 1, "two ranks")


@pytest.mark.parametrize("extra", [["--rtm_f16"], ["--rtm_format", "sparse"]], ids=["f16", "sparse"])
def test_cli_holdout_storages(tmp_path, binary, extra):  # noqa: F811
    case = _case(tmp_path)
    prof = str(tmp_path / "profile.jsonl")
    d = _read(_run(tmp_path, binary, case, "st.h5", extra=[*extra, "--profile", prof]))
    assert np.all(np.isfinite(d["value"])) and np.all(np.isfinite(d["sums"])) and np.all(d["eligible"] == 1)
    check_scores_and_solution(d, 1, " ".join(extra))
    recs = [json.loads(line) for line in open(prof)]
    assert recs[0]["load"] is True and recs[0]["solver_path"].startswith("multi-frame")
    assert [r for r in recs if r.get("series")] and recs[-1].get("holdout") is True
    assert list(recs[-1]) == ["holdout", "mode", "folds", "seed", "betas", "frames", "columns", "groups",
                              "scoring_kernel_ms", "ms"]
    h = recs[-1]
    assert (h["mode"], h["folds"], h["seed"], h["betas"], h["frames"], h["columns"]) == ("pixels", K, 0, 3, T, 30)
    assert h["groups"] == -(-30 // (4 if extra == ["--rtm_f16"] else 8)) and h["scoring_kernel_ms"] > 0 and h["ms"] > 0
