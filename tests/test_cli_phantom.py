"""sartsolver --phantom end to end on the fixture of tests/test_cli_replicas.py (two cameras, one stored sparse, a
Laplacian) with three phantoms -- a smooth blob, two isolated voxels, all zeros: every dataset of /phantom, the
noise-free projections against NumPy fp64 A t (tests/fit_bound.py), every stored column against the fp64 oracle run on
the stored image row (with --replicas: on its NumPy perturbation at the stored time, utils/philox.py) for the column's
recorded update count, the sums against NumPy on the stored columns within the kernel's bound, the scores against the
NumPy restatement bit for bit, /solution against column 0; on two ranks sharing the GPU; on f16 and sparse storage.

The measured frames of the fixture are never solved: the runs would not match these oracles if they were."""
import json
import math
import os

import numpy as np
import pytest

from fit_bound import assert_image, reference
from fp32_bound import fp32_errors
from mpi_cuda_sartsolver_amd.io.fixtures import make_case, write_phantom_file
from mpi_cuda_sartsolver_amd.ops import native
from mpi_cuda_sartsolver_amd.utils import philox
from test_cli_e2e import CLI_FP32_FACTOR, _laplacian
from test_gpu_moments import check_moments
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

pytestmark = pytest.mark.gpu

NP, N, NVOXEL, BETA, REL, ITERS = 3, 3, 2048, 1e-2, 0.02, 60
TIMES = np.array([0.25, 0.5, 2.0])
SCORES = ("rel_l2", "cosine", "total_ratio", "peak_ratio", "max_error", "inside_fraction")
F64 = ("image", "time", "sums", *SCORES)
I32 = ("status", "iterations")
PROFILE_KEYS = ["phantom", "phantoms", "replicas", "groups", "projection_kernel_ms", "scoring_kernel_ms"]


def _case(tmp_path):
    return make_case(str(tmp_path / "c"), sparse_cameras=("cam_b",), laplacian=True, nframes=2, saturate=0.05,
                     nvoxel=NVOXEL, grid=(16, 16, 16), shapes=((24, 32), (20, 30)))


def _truths():
    """[3, nvoxel]: a blob that is smooth in the voxel order (the fixture's Laplacian is the chain over it), two
    isolated voxels, the dark frame."""
    v = np.arange(NVOXEL, dtype=np.float64)
    t = np.zeros((NP, NVOXEL))
    t[0] = np.exp(-((v - 1000.0) / 180.0) ** 2)
    t[0][t[0] < 1e-3] = 0.0
    t[1, 300], t[1, 1500] = 1.0, 2.5
    return t


def _noise(case):
    """(abs, shot, rel): the floor and the shot coefficient at 1e-3 of the blob's brightest pixel."""
    top = float((case.A.astype(np.float64) @ _truths()[0]).max())
    return 1e-3 * top, 1e-3 * top, REL


def _run(tmp_path, binary, case, name, nrep=0, extra=(), nproc=1, iters=ITERS):  # noqa: F811
    out = str(tmp_path / name)
    ph = write_phantom_file(str(tmp_path / "truth.h5"), _truths(), time=TIMES)
    argv = ["--phantom", ph, "-m", str(iters), "-c", "1e-12", "-l", case.laplacian_file, "-b", repr(BETA)]
    if nrep:
        a, s, r = _noise(case)
        argv += ["--replicas", str(nrep), "--replicas_keep", "--noise_abs", repr(a), "--noise_shot", repr(s),
                 "--noise_rel", repr(r), "--noise_seed", "5"]
    res = _run_native(binary, [*argv, *extra, "-o", out, *case.files], nproc=nproc)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count("Processed in:") == NP, res.stdout
    assert f"Frames processed: {NP} " in res.stdout, res.stdout
    return out


def _read(path, nrep):
    n = native()
    d = {k: n.read_dataset_f64(path, "phantom/" + k) for k in F64 + I32}
    for k in ("value", "status", "iterations", "time"):
        d["solution/" + k] = n.read_dataset_f64(path, "solution/" + k)
    # the stored columns [NP, nc, nvoxel]: /uncertainty/value with --replicas_keep, else /solution is column 0
    d["columns"] = n.read_dataset_f64(path, "uncertainty/value") if nrep else d["solution/value"][:, None, :]
    return d


def check_layout(out, d, nrep):
    """Check 1: names, stored types, shapes; the times."""
    n, nc = native(), nrep + 1
    npixel = d["image"].shape[1]
    shapes = {"image": (NP, npixel), "time": (NP,), "sums": (NP, nc, 10)}
    for name in F64 + I32:
        assert n.dataset_dtype(out, "phantom/" + name) == ("<i4" if name in I32 else "<f8"), name
        assert d[name].shape == shapes.get(name, (NP, nc)), name
    assert np.array_equal(d["time"], TIMES) and np.array_equal(d["solution/time"], d["time"])
    assert d["solution/value"].shape == (NP, NVOXEL) and d["columns"].shape == (NP, nc, NVOXEL)
    assert n.read_dataset_f64(out, "voxel_map/i").size > 0  # the voxel map is copied as in any run
    assert np.all(d["iterations"] >= 1) and np.all(d["iterations"] <= ITERS)


def check_image(case, d, what):
    """Check 2: the stored projections against NumPy fp64 A t."""
    F_ref, bound = reference(case.A, _truths())
    assert d["image"].shape == F_ref.shape
    assert_image(d["image"], F_ref, bound, what)
    assert np.array_equal(d["image"][2], np.zeros(F_ref.shape[1]))  # the dark frame


def check_columns(case, d, nrep, what):
    """Check 3: every stored column against the oracle on the stored image row (replica r: its NumPy perturbation at
    the stored time, over the global pixel indices) for the column's recorded update count."""
    L = _laplacian(case)
    a, s, r = _noise(case)
    for k in range(NP):
        G = philox.perturb(d["image"][k], float(d["time"][k]), nrep, a, s, r, 5) if nrep else d["image"][k][None, :]
        for c in range(nrep + 1):
            it, x = int(d["iterations"][k, c]), d["columns"][k, c]
            assert np.all(np.isfinite(x)), (k, c)
            # (the dark frame too: the cold start's floor of 1e-7 decays under the updates, in the oracle as on the GPU)
            e, e32 = fp32_errors(x, case.A, G[c], L, iterations=it, beta_laplace=BETA)
            print(f"{what} phantom {k} column {c}: {it} updates, rel {e:.3e} fp32 emulation {e32:.3e}")
            assert e <= CLI_FP32_FACTOR * e32 + 1e-6, (k, c, e, e32)


def check_scores(d, nrep, what):
    """Checks 4 and 5: the sums against fsum of NumPy's terms on the stored columns within the kernel's bound (the
    maxima exactly), the scores against the NumPy restatement bitwise, /solution is column 0."""
    from mpi_cuda_sartsolver_amd.models.phantom import phantom_scores

    T = _truths()
    for k in range(NP):
        for c in range(nrep + 1):
            x, t, got = d["columns"][k, c], T[k], d["sums"][k, c]
            dd = x - t
            for q, term in enumerate([t, x, t * t, x * x, x * t, dd * dd, np.where(t > 0, x, 0.0)]):
                bound = (NVOXEL + 4) * 2.0 ** -53 * math.fsum(np.abs(term))
                assert abs(float(got[q]) - math.fsum(term)) <= bound, (what, k, c, q)
            assert got[7] == np.abs(dd).max() and got[8] == t.max() and got[9] == x.max(), (what, k, c)
    want = phantom_scores(d["sums"])
    for name in SCORES:
        assert np.array_equal(d[name], want[name], equal_nan=True), (what, name)
    assert np.all(np.isnan(d["rel_l2"][2])) and np.all(np.isnan(d["cosine"][2]))  # the dark truth: no denominator
    assert np.all(np.isfinite(d["rel_l2"][:2])) and np.all(d["cosine"][:2] > 0.0)
    for k in range(NP):
        assert np.array_equal(d["solution/value"][k], d["columns"][k, 0]), k
        assert int(d["solution/status"][k]) == int(d["status"][k, 0])
        assert int(d["solution/iterations"][k]) == int(d["iterations"][k, 0])


def test_cli_phantom(tmp_path, binary):  # noqa: F811
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics

    case = _case(tmp_path)
    out = _run(tmp_path, binary, case, "ph.h5")
    d = _read(out, 0)
    check_layout(out, d, 0)
    check_image(case, d, "one rank")
    check_columns(case, d, 0, "one rank")
    check_scores(d, 0, "one rank")
    # check 8, the physics on the oracle alone: on the blob without noise more updates come closer to the truth, and
    # the file's score at 60 updates is the oracle's
    L, t = _laplacian(case), _truths()[0]
    rel = [float(np.linalg.norm(sart_gpu_semantics(case.A, d["image"][0], L, conv_tolerance=0.0, beta_laplace=BETA,
                                                   max_iterations=m)[0] - t) / np.linalg.norm(t)) for m in (5, 20, 60)]
    print(f"oracle rel_l2 at 5, 20, 60 updates: {rel}; the file's: {d['rel_l2'][0, 0]:.6e} "
          f"({int(d['iterations'][0, 0])} updates)")
    assert rel[0] > rel[1] > rel[2]
    assert int(d["iterations"][0, 0]) == ITERS
    assert abs(d["rel_l2"][0, 0] - rel[2]) <= 0.01 * rel[2]


def test_cli_phantom_replicas(tmp_path, binary):  # noqa: F811
    case = _case(tmp_path)
    out = _run(tmp_path, binary, case, "rep.h5", nrep=N)
    d = _read(out, N)
    check_layout(out, d, N)
    check_image(case, d, "replicas")
    check_columns(case, d, N, "replicas")
    check_scores(d, N, "replicas")
    # /uncertainty exactly as in a replica run: the moments of the stored replicas
    n = native()
    mean, std, count = (n.read_dataset_f64(out, "uncertainty/" + k) for k in ("mean", "std", "count"))
    assert np.array_equal(n.read_dataset_f64(out, "uncertainty/iterations"), d["iterations"])
    for k in range(NP):
        assert int(count[k]) == N
        check_moments(mean[k], std[k], d["columns"][k, 1:], np.ones(N, dtype=np.uint8), f"phantom {k}")
    # the dark frame: the noise floor alone leaves a positive reconstruction (the clamp's bias)
    assert np.all(d["sums"][2, 1:, 1] > 0.0) and np.all(d["sums"][2, :, 0] == 0.0)
    # the noise-free columns know no noise: the run without replicas gives the same bits
    d0 = _read(_run(tmp_path, binary, case, "ph.h5"), 0)
    assert np.array_equal(d0["image"], d["image"]) and np.array_equal(d0["columns"][:, 0], d["columns"][:, 0])
    assert np.array_equal(d0["sums"][:, 0], d["sums"][:, 0])


def test_cli_phantom_two_ranks_one_device(tmp_path, binary):  # noqa: F811
    """Check 6: two ranks on one GPU (staged reductions over TCP, as test_cli_replicas_two_ranks_one_device launches)
    project the same bits per pixel -- the fit kernels' guarantee -- and the second rank's replicas carry their global
    pixel indices."""
    case = _case(tmp_path)
    one = _read(_run(tmp_path, binary, case, "one.h5", nrep=N), N)
    saved = {k: os.environ.get(k) for k in ("SART_DIST_BACKEND", "SART_P2P")}
    os.environ["SART_DIST_BACKEND"] = "tcp"
    os.environ["SART_P2P"] = "0"
    try:
        out = _run(tmp_path, binary, case, "two.h5", nrep=N, nproc=2)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    d = _read(out, N)
    assert np.array_equal(d["image"], one["image"])
    check_layout(out, d, N)
    check_columns(case, d, N, "two ranks")
    check_scores(d, N, "two ranks")


@pytest.mark.parametrize("extra", [["--rtm_f16"], ["--rtm_format", "sparse"]], ids=["f16", "sparse"])
def test_cli_phantom_storages(tmp_path, binary, extra):  # noqa: F811
    """Check 7: the other storages of the batch engine (their solver bounds are tested elsewhere); --profile."""
    case = _case(tmp_path)
    prof = str(tmp_path / "profile.jsonl")
    out = _run(tmp_path, binary, case, "st.h5", nrep=N, extra=[*extra, "--profile", prof])
    d = _read(out, N)
    check_layout(out, d, N)
    assert np.all(np.isfinite(d["columns"])) and np.all(np.isfinite(d["image"])) and np.all(np.isfinite(d["sums"]))
    check_scores(d, N, " ".join(extra))
    if extra[0] == "--rtm_format":  # the matrix as stored is the fp32 one (the f16 shard projects its quantised one)
        check_image(case, d, "sparse")
    # --profile: the load line, the series line, the uncertainty line as in any replica run, then one phantom line
    recs = [json.loads(line) for line in open(prof)]
    assert recs[0]["load"] is True and recs[0]["solver_path"].startswith("multi-frame")
    assert [r for r in recs if r.get("series")] and len([r for r in recs if r.get("phantom")]) == 1
    assert recs[-2].get("uncertainty") is True and recs[-1].get("phantom") is True
    assert list(recs[-1]) == PROFILE_KEYS
    p = recs[-1]
    assert (p["phantoms"], p["replicas"], p["groups"]) == (NP, N, 1)
    assert p["projection_kernel_ms"] > 0 and p["scoring_kernel_ms"] > 0
