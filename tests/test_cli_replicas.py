"""sartsolver --replicas end to end on the fixture of tests/test_cli_beta_scan.py with two frames (two cameras, one
stored sparse, a Laplacian, saturated pixels): every dataset of /uncertainty, every stored column against the fp64
oracle run on the NumPy-perturbed frame (utils/philox.py) for the column's recorded update count, the moments against
the NumPy loop on the stored columns, /solution against column 0; with another seed, on two ranks sharing the GPU
(global pixel indices), and on f16 and sparse storage.

Not tested: the driver's refusal of 2^32 pixels and more ("Argument replicas applies to fewer than 2^32 pixels"). It
reads the count from the input files' metadata after they validate, and an RTM and images with 2^32 rows are no fixture
for a test; the kernel launcher's own refusal of a pixel index beyond 2^32 is in tests/test_gpu_noise.py."""
import os

import numpy as np
import pytest

from fp32_bound import fp32_errors
from mpi_cuda_sartsolver_amd.io.fixtures import make_case
from mpi_cuda_sartsolver_amd.ops import native
from mpi_cuda_sartsolver_amd.utils import philox
from test_cli_e2e import CLI_FP32_FACTOR, _frames, _laplacian
from test_gpu_moments import check_moments
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

pytestmark = pytest.mark.gpu

T, N, NVOXEL, BETA, REL = 2, 7, 2048, 1e-2, 0.02
TYPES = {"mean": "<f8", "std": "<f8", "count": "<i4", "status": "<i4", "iterations": "<i4", "noise": "<f8",
         "seed": "<u8", "value": "<f8"}


def _case(tmp_path):
    return make_case(str(tmp_path / "c"), sparse_cameras=("cam_b",), laplacian=True, nframes=T, saturate=0.05,
                     nvoxel=NVOXEL, grid=(16, 16, 16), shapes=((24, 32), (20, 30)))


def _noise(case):
    """(abs, shot, rel): the floor and the shot coefficient at 1e-3 of the frames' maximum."""
    top = max(float(f.max()) for f in _frames(case))
    return 1e-3 * top, 1e-3 * top, REL


def _times(case):
    return np.asarray(next(iter(case.times.values())), dtype=np.float64)


def _run(tmp_path, binary, case, name, seed=0, extra=(), nproc=1):  # noqa: F811
    out = str(tmp_path / name)
    a, s, r = _noise(case)
    argv = ["--replicas", str(N), "--replicas_keep", "-m", "60", "-c", "1e-6", "--noise_abs", repr(a), "--noise_shot",
            repr(s), "--noise_rel", repr(r), "--noise_seed", str(seed), "-l", case.laplacian_file, "-b", repr(BETA),
            *extra, "-o", out, *case.files]
    res = _run_native(binary, argv, nproc=nproc)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count("Processed in:") == T, res.stdout
    return out


def _read(path):
    n = native()
    d = {k: n.read_dataset_f64(path, "uncertainty/" + k) for k in TYPES if k != "seed"}
    for k in ("value", "status", "iterations", "time"):
        d["solution/" + k] = n.read_dataset_f64(path, "solution/" + k)
    return d


def _perturbed(case, seed, times):
    """[T][N + 1, npixel]: the frames the driver must have solved, by the NumPy emulation at the stored times (the
    doubles of /solution/time: their bits are part of the counter)."""
    a, s, r = _noise(case)
    return [philox.perturb(g, float(t), N, a, s, r, seed) for g, t in zip(_frames(case), times)]


def check_columns(case, d, seed, what):
    """Check 2: every stored column against the oracle on the NumPy-perturbed frame, at the beta-scan column rule.
    Returns the fp32 emulation's errors [T, N + 1]."""
    L, G = _laplacian(case), _perturbed(case, seed, d["solution/time"])
    e32s = np.zeros((T, N + 1))
    for k in range(T):
        for r in range(N + 1):
            it = int(d["iterations"][k, r])
            e, e32 = fp32_errors(d["value"][k, r], case.A, G[k][r], L, iterations=it, beta_laplace=BETA)
            e32s[k, r] = e32
            print(f"{what} frame {k} replica {r}: {it} updates, rel {e:.3e} fp32 emulation {e32:.3e}")
            assert e <= CLI_FP32_FACTOR * e32 + 1e-6, (k, r, e, e32)
    return e32s


def check_moments_and_solution(d, what):
    """Checks 3 and 4: mean, std and count against NumPy on the stored columns; /solution is column 0."""
    for k in range(T):
        use = np.ones(N, dtype=np.uint8)
        assert int(d["count"][k]) == N
        check_moments(d["mean"][k], d["std"][k], d["value"][k, 1:], use, f"{what} frame {k}")
        assert np.array_equal(d["solution/value"][k], d["value"][k, 0]), k
        assert int(d["solution/status"][k]) == int(d["status"][k, 0])
        assert int(d["solution/iterations"][k]) == int(d["iterations"][k, 0])


def test_cli_replicas(tmp_path, binary):  # noqa: F811
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics

    case = _case(tmp_path)
    out = _run(tmp_path, binary, case, "rep.h5")
    n = native()
    d = _read(out)
    # check 1: names, stored types, shapes; the noise and the seed as given
    shapes = {"mean": (T, NVOXEL), "std": (T, NVOXEL), "count": (T,), "noise": (3,), "seed": (1,),
              "value": (T, N + 1, NVOXEL)}
    for name, dtype in TYPES.items():
        assert n.dataset_dtype(out, "uncertainty/" + name) == dtype, name
        if name != "seed":
            assert d[name].shape == shapes.get(name, (T, N + 1)), name
    np.testing.assert_array_equal(d["noise"], _noise(case))
    assert [int(v) for v in n.read_dataset_f64(out, "uncertainty/seed")] == [0]
    assert d["solution/value"].shape == (T, NVOXEL)
    np.testing.assert_allclose(d["solution/time"], _times(case), atol=1e-12)
    assert n.read_dataset_f64(out, "voxel_map/i").size > 0  # the voxel map is copied as in any run
    assert np.all(np.isfinite(d["value"])) and np.all(d["iterations"] >= 1) and np.all(d["iterations"] <= 60)
    e32 = check_columns(case, d, 0, "one rank")
    check_moments_and_solution(d, "one rank")
    # check 5, the precondition: the spread the noise causes is far above what fp32 solves differ by, on the oracle's
    # own replicas
    L, G = _laplacian(case), _perturbed(case, 0, d["solution/time"])
    for k in range(T):
        X = np.stack([sart_gpu_semantics(case.A, G[k][r], L, conv_tolerance=0.0, beta_laplace=BETA,
                                         max_iterations=int(d["iterations"][k, r]))[0] for r in range(N + 1)])
        spread, x0 = np.linalg.norm(X[1:].std(axis=0, ddof=1)), np.linalg.norm(X[0])
        print(f"frame {k}: oracle ||std|| / ||x0|| = {spread / x0:.3e}, 100 max e32 = {100 * e32[k].max():.3e}")
        assert spread >= 100 * e32[k].max() * x0
        # and the file's spread is that spread
        assert abs(np.linalg.norm(d["std"][k]) - spread) <= 0.01 * spread


def test_cli_replicas_another_seed(tmp_path, binary):  # noqa: F811
    """Check 6."""
    case = _case(tmp_path)
    d0 = _read(_run(tmp_path, binary, case, "s0.h5"))
    out = _run(tmp_path, binary, case, "s1.h5", seed=1)
    d1 = _read(out)
    assert [int(v) for v in native().read_dataset_f64(out, "uncertainty/seed")] == [1]
    assert not np.array_equal(d1["std"], d0["std"]) and not np.array_equal(d1["value"][:, 1:], d0["value"][:, 1:])
    assert np.array_equal(d1["value"][:, 0], d0["value"][:, 0])  # the nominal column knows no seed
    check_columns(case, d1, 1, "seed 1")
    check_moments_and_solution(d1, "seed 1")


def test_cli_replicas_two_ranks_one_device(tmp_path, binary):  # noqa: F811
    """Check 7: two ranks on one GPU (staged reductions over TCP, as test_cli_fp64_two_ranks_one_device launches)
    against the same NumPy frames: the second rank's pixels carry their global indices."""
    case = _case(tmp_path)
    saved = {k: os.environ.get(k) for k in ("SART_DIST_BACKEND", "SART_P2P")}
    os.environ["SART_DIST_BACKEND"] = "tcp"
    os.environ["SART_P2P"] = "0"
    try:
        out = _run(tmp_path, binary, case, "two.h5", nproc=2)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    d = _read(out)
    check_columns(case, d, 0, "two ranks")
    check_moments_and_solution(d, "two ranks")


@pytest.mark.parametrize("extra", [["--rtm_f16"], ["--rtm_format", "sparse"]], ids=["f16", "sparse"])
def test_cli_replicas_storages(tmp_path, binary, extra):  # noqa: F811
    """Check 8: the other storages of the batch engine (their solver bounds are tested elsewhere)."""
    import json

    case = _case(tmp_path)
    prof = str(tmp_path / "profile.jsonl")
    d = _read(_run(tmp_path, binary, case, "st.h5", extra=[*extra, "--profile", prof]))
    assert np.all(np.isfinite(d["value"])) and np.all(d["count"] == N)
    check_moments_and_solution(d, " ".join(extra))
    # --profile: the load line's solver path as in any batched run, the series line, then one uncertainty line
    recs = [json.loads(line) for line in open(prof)]
    assert recs[0]["load"] is True and recs[0]["solver_path"].startswith("multi-frame")
    assert [r for r in recs if r.get("series")] and recs[-1].get("uncertainty") is True
    assert list(recs[-1]) == ["uncertainty", "replicas", "seed", "noise_abs", "noise_shot", "noise_rel",
                              "noise_kernel_ms", "moments_kernel_ms", "frames"]
    a, s, r = _noise(case)
    u = recs[-1]
    assert (u["replicas"], u["seed"], u["frames"]) == (N, 0, T) and u["noise_rel"] == r
    assert u["noise_abs"] == pytest.approx(a, rel=1e-5) and u["noise_shot"] == pytest.approx(s, rel=1e-5)
    assert u["noise_kernel_ms"] > 0 and u["moments_kernel_ms"] > 0
