"""sartsolver --fit / --fit_only on the GPU, end to end on the fixture case of tests/test_cli_fp64.py (two cameras, one
stored sparse, a Laplacian, 3 frames with saturated pixels): /fit/image[k] against A_stored @ value[k] with value[k]
read from the same file, every statistic and the per-camera split against NumPy (tests/fit_bound.py), for every
storage and solver; --fit_only bitwise on one rank and two, and across storages; --resume --fit; and that the added
group changes nothing else in the file."""
import json
import os
import shutil

import numpy as np
import pytest

import fit_bound as fb
from mpi_cuda_sartsolver_amd.io.fixtures import make_case
from mpi_cuda_sartsolver_amd.ops import native
from mpi_cuda_sartsolver_amd.utils.f16rows import quantise_rows_f16
from test_cli_e2e import _frames
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

pytestmark = pytest.mark.gpu


def _camera_pixels(case):
    return [int(case.masks[c].sum()) for c in sorted(case.masks)]


@pytest.fixture(scope="module")
def dense(tmp_path_factory, binary):  # noqa: F811
    """The case, its solver options, and the output of the default --fit run (shared, never modified)"""
    d = tmp_path_factory.mktemp("cli_fit")
    case = make_case(str(d / "case"), sparse_cameras=("cam_b",), laplacian=True, nframes=3, saturate=0.05)
    base = ["-m", "80", "-c", "1e-7", "-l", case.laplacian_file, "-b", "1e-3"]
    out, prof = str(d / "default.h5"), str(d / "default.jsonl")
    r = _run_native(binary, base + ["--fit", "--profile", prof, "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    return d, case, base, out, prof


def _check(path, case, A_stored, what, nterms=None):
    return fb.check_fit_file(native(), path, A_stored, _frames(case), _camera_pixels(case), nterms=nterms, what=what)


def test_cli_fit_defaults(dense):
    d, case, base, out, prof = dense
    _check(out, case, case.A, "defaults")
    recs = [json.loads(line) for line in open(prof)]
    rec = recs[-1]
    assert rec["fit"] is True and rec["frames"] == 3 and rec["groups"] == 1 and rec["ranks"] == 1, rec
    assert rec["rtm_storage"] == "fp32" and rec["rtm_format"] == "dense" and rec["fit_ms"] > 0
    assert sum(1 for r in recs if r.get("fit")) == 1


@pytest.mark.parametrize("extra, stored", [
    (["--rtm_bf16"], "bf16"), (["--rtm_f16"], "f16"), (["--batch_frames", "16"], "fp32"), (["--fp64"], "fp32"),
    (["--partition_voxels"], "fp32"), (["--two_pass"], "fp32")], ids=lambda v: " ".join(v) if isinstance(v, list) else "")
def test_cli_fit_storages_and_solvers(dense, binary, extra, stored):  # noqa: F811
    d, case, base, _, _ = dense
    out = str(d / ("fit_" + "_".join(e.strip("-") for e in extra) + ".h5"))
    r = _run_native(binary, base + extra + ["--fit", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Fit of 3 frame(s)" in r.stdout
    A = {"fp32": case.A, "bf16": fb.round_bf16(case.A), "f16": np.asarray(quantise_rows_f16(case.A)[2])}[stored]
    _check(out, case, A, " ".join(extra))


def test_cli_fit_sparse(tmp_path, binary):  # noqa: F811
    case = make_case(str(tmp_path / "c"), shapes=((8, 8), (8, 8)), grid=(6, 6, 6), raytraced=True, direct_only=True,
                     sparse_cameras=("cam_a", "cam_b"), nframes=3, saturate=0.02)
    out, prof = str(tmp_path / "s.h5"), str(tmp_path / "s.jsonl")
    r = _run_native(binary, ["-m", "40", "-c", "1e-6", "--rtm_format", "sparse", "--fit", "--profile", prof, "-o", out,
                             *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sparse: " in r.stdout
    _check(out, case, case.A, "sparse", nterms=np.count_nonzero(case.A, axis=1))
    rec = [json.loads(line) for line in open(prof)][-1]
    assert rec["fit"] is True and rec["rtm_format"] == "sparse" and rec["rtm_storage"] == "fp32", rec


def _two_ranks_one_gpu(binary, args):  # noqa: F811
    saved = {k: os.environ.get(k) for k in ("SART_DIST_BACKEND", "SART_P2P")}
    os.environ["SART_DIST_BACKEND"] = "tcp"
    os.environ["SART_P2P"] = "0"
    try:
        return _run_native(binary, args, nproc=2)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_cli_fit_sparse_bitwise_one_and_two_ranks(tmp_path, binary):  # noqa: F811
    """The CSR shard: --fit on one rank, then --fit_only (no engine) on one rank and on two ranks of one GPU, whose
    shards have other mean row lengths than the whole matrix: every /fit dataset equal"""
    case = make_case(str(tmp_path / "c"), shapes=((8, 8), (8, 8)), grid=(6, 6, 6), raytraced=True, direct_only=True,
                     sparse_cameras=("cam_a", "cam_b"), nframes=3, saturate=0.02)
    nnz = np.count_nonzero(case.A, axis=1)
    half = case.npixel - case.npixel // 2  # rank 0's rows of two
    assert nnz[:half].mean() != nnz[half:].mean()
    out = str(tmp_path / "s.h5")
    r = _run_native(binary, ["-m", "40", "-c", "1e-6", "--rtm_format", "sparse", "--fit", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    n = native()
    first = fb.read_fit(n, out)
    for ranks in (1, 2):
        path = str(tmp_path / f"only{ranks}.h5")
        shutil.copy(out, path)
        args = ["--rtm_format", "sparse", "--fit_only", "-o", path, *case.files]
        r = _run_native(binary, args) if ranks == 1 else _two_ranks_one_gpu(binary, args)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "sparse: " in r.stdout and "Processed in:" not in r.stdout
        got = fb.read_fit(n, path)
        for k in fb.FIT_DATASETS + ("value", "time"):
            np.testing.assert_array_equal(got[k], first[k], err_msg=f"{k}, {ranks} rank(s)")
    _check(path, case, case.A, "sparse, two ranks", nterms=nnz)


@pytest.mark.parametrize("extra", [[], ["--rtm_bf16"]], ids=["fp32", "bf16"])
def test_cli_fit_does_not_depend_on_the_group_size(dense, binary, extra):  # noqa: F811
    """The driver's solutions per pass (8, 4 on 16-bit shards; SART_FIT_GROUP) change nothing in the file"""
    d, case, base, out, _ = dense
    n = native()
    files = {}
    for group in ("", "1", "2"):
        path = str(d / f"group{group}_{len(extra)}.h5")
        shutil.copy(out, path)
        saved = os.environ.get("SART_FIT_GROUP")
        if group:
            os.environ["SART_FIT_GROUP"] = group
        try:
            r = _run_native(binary, extra + ["--fit_only", "--profile", path + ".jsonl", "-o", path, *case.files])
        finally:
            os.environ.pop("SART_FIT_GROUP", None)
            if saved is not None:
                os.environ["SART_FIT_GROUP"] = saved
        assert r.returncode == 0, r.stdout + r.stderr
        rec = [json.loads(line) for line in open(path + ".jsonl")][-1]
        assert rec["fit"] and rec["groups"] == {"": 1, "1": 3, "2": 2}[group], rec
        files[group] = fb.read_fit(n, path)
    for group in ("1", "2"):
        for k in fb.FIT_DATASETS:
            np.testing.assert_array_equal(files[group][k], files[""][k], err_msg=f"{k}, groups of {group}")


def test_cli_fit_adds_a_group_and_nothing_else(dense, binary):  # noqa: F811
    d, case, base, out, _ = dense
    plain = str(d / "plain.h5")
    r = _run_native(binary, base + ["-o", plain, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Fit of" not in r.stdout
    n = native()
    for k in ("value", "time", "status", "iterations", "time_cam_a", "time_cam_b"):
        np.testing.assert_array_equal(n.read_dataset_f64(out, "solution/" + k), n.read_dataset_f64(plain, "solution/" + k))
    with pytest.raises(RuntimeError):
        n.read_dataset_f64(plain, "fit/image")


def test_cli_fit_only_bitwise_one_and_two_ranks(dense, binary):  # noqa: F811
    """--fit_only over one file on one rank and on two ranks of one GPU (staged TCP): every /fit dataset equal"""
    d, case, base, out, _ = dense
    n = native()
    first = fb.read_fit(n, out)
    a, b = str(d / "only1.h5"), str(d / "only2.h5")
    shutil.copy(out, a)
    shutil.copy(out, b)
    r = _run_native(binary, ["--fit_only", "-o", a, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Processed in:" not in r.stdout and "Fit of 3 frame(s)" in r.stdout
    r = _two_ranks_one_gpu(binary, ["--fit_only", "-o", b, *case.files])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    one, two = fb.read_fit(n, a), fb.read_fit(n, b)
    for k in fb.FIT_DATASETS + ("value", "time"):
        np.testing.assert_array_equal(one[k], two[k], err_msg=k)
        np.testing.assert_array_equal(one[k], first[k], err_msg=k)  # and equal to the --fit run's own pass


def test_cli_fit_only_across_storages(dense, binary):  # noqa: F811
    """A --rtm_bf16 solution measured against the fp32 matrix"""
    d, case, base, _, _ = dense
    out = str(d / "bf16_then_fp32.h5")
    r = _run_native(binary, base + ["--rtm_bf16", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run_native(binary, ["--fit_only", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    _check(out, case, case.A, "fp32 fit of a bf16 solution")


def test_cli_resume_fit_covers_every_frame(dense, binary):  # noqa: F811
    d, case, base, _, _ = dense
    out = str(d / "resume.h5")
    r = _run_native(binary, base + ["--fit", "-t", "0:0.15", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert native().read_dataset_f64(out, "fit/image").shape[0] == 2
    r = _run_native(binary, base + ["--resume", "--fit", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("Processed in:") == 1 and "Fit of 3 frame(s)" in r.stdout
    got = _check(out, case, case.A, "resume")
    # the rows of the resumed run are those of a fresh pass over the same solutions, bit for bit
    again = str(d / "resume_again.h5")
    shutil.copy(out, again)
    r = _run_native(binary, ["--fit_only", "-o", again, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    fresh = fb.read_fit(native(), again)
    for k in fb.FIT_DATASETS + ("value", "time"):
        np.testing.assert_array_equal(fresh[k], got[k], err_msg=k)
