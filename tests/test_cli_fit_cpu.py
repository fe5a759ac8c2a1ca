"""sartsolver --use_cpu --fit / --fit_only end to end (no GPU): the /fit group of the output file against
A @ value[k] with value[k] read from the same file and the statistics in NumPy (tests/fit_bound.py), dense and sparse
shards, one rank and two (TCP), and the errors: no output file to fit, a stored time outside --time_range."""
import json
import shutil

import numpy as np
import pytest

import fit_bound as fb
from mpi_cuda_sartsolver_amd.io.fixtures import make_case
from mpi_cuda_sartsolver_amd.ops import native
from test_cli_e2e import _frames
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

BASE = ["--use_cpu", "-m", "40", "-c", "1e-6"]


def _camera_pixels(case):
    return [int(case.masks[c].sum()) for c in sorted(case.masks)]


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    d = tmp_path_factory.mktemp("fit_dense")
    case = make_case(str(d / "case"), sparse_cameras=("cam_b",), laplacian=True, nframes=3, saturate=0.05)
    return d, case


@pytest.fixture(scope="module")
def sparse(tmp_path_factory):
    d = tmp_path_factory.mktemp("fit_sparse")
    case = make_case(str(d / "case"), shapes=((8, 8), (8, 8)), grid=(6, 6, 6), raytraced=True, direct_only=True,
                     sparse_cameras=("cam_a", "cam_b"), nframes=3, saturate=0.02)
    return d, case


def _same_fit(a, b):
    for k in fb.FIT_DATASETS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_cli_cpu_fit_dense_one_and_two_ranks(dense, binary):  # noqa: F811
    d, case = dense
    out, plain, prof = str(d / "fit.h5"), str(d / "plain.h5"), str(d / "p.jsonl")
    args = BASE + ["-l", case.laplacian_file, "-b", "1e-3"]
    r = _run_native(binary, args + ["--fit", "--profile", prof, "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Fit of 3 frame(s)" in r.stdout
    got = fb.check_fit_file(native(), out, case.A, _frames(case), _camera_pixels(case), what="cpu dense")
    # the added group changes nothing else
    r = _run_native(binary, args + ["-o", plain, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    n = native()
    for k in ("value", "time", "status", "iterations"):
        np.testing.assert_array_equal(n.read_dataset_f64(out, "solution/" + k), n.read_dataset_f64(plain, "solution/" + k))
    with pytest.raises(RuntimeError):
        n.read_dataset_f64(plain, "fit/image")
    rec = [json.loads(line) for line in open(prof)][-1]
    assert rec["fit"] is True and rec["frames"] == 3 and rec["groups"] == 1 and rec["ranks"] == 1, rec
    assert rec["rtm_storage"] == "fp32" and rec["rtm_format"] == "dense" and rec["fit_ms"] > 0
    # --fit_only over the same file: one rank and two give the same group bit for bit, and replace the one there
    r = _run_native(binary, ["--use_cpu", "--fit_only", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Processed in:" not in r.stdout
    one = fb.read_fit(n, out)
    _same_fit(one, got)
    r = _run_native(binary, ["--use_cpu", "--fit_only", "-o", out, *case.files], nproc=2)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    two = fb.read_fit(n, out)
    _same_fit(two, one)
    np.testing.assert_array_equal(two["value"], got["value"])


def test_cli_cpu_fit_two_ranks_solve(dense, binary):  # noqa: F811
    d, case = dense
    out = str(d / "two.h5")
    r = _run_native(binary, BASE + ["--fit", "-o", out, *case.files], nproc=2)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    fb.check_fit_file(native(), out, case.A, _frames(case), _camera_pixels(case), what="cpu dense, two ranks")


@pytest.mark.parametrize("nproc", [1, 2])
def test_cli_cpu_fit_sparse(sparse, binary, nproc):  # noqa: F811
    d, case = sparse
    out = str(d / f"fit{nproc}.h5")
    r = _run_native(binary, BASE + ["--rtm_format", "sparse", "--fit", "-o", out, *case.files], nproc=nproc)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    nterms = np.count_nonzero(case.A, axis=1)
    got = fb.check_fit_file(native(), out, case.A, _frames(case), _camera_pixels(case), nterms=nterms,
                            what=f"cpu sparse, {nproc} rank(s)")
    # --fit_only on the CSR shard (no solver is built): one rank and two, bit for bit each other's and the --fit run's
    only = {}
    for ranks in (1, 2):
        path = str(d / f"only{nproc}_{ranks}.h5")
        shutil.copy(out, path)
        r = _run_native(binary, ["--use_cpu", "--rtm_format", "sparse", "--fit_only", "-o", path, *case.files],
                        nproc=ranks)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "Processed in:" not in r.stdout
        only[ranks] = fb.read_fit(native(), path)
        for k in fb.FIT_DATASETS + ("value", "time"):
            np.testing.assert_array_equal(only[ranks][k], got[k], err_msg=f"{k}, {ranks} rank(s)")
    # the sparse solution against the dense loader: --fit_only with the other format on the same file
    r = _run_native(binary, ["--use_cpu", "--rtm_format", "dense", "--fit_only", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    again = fb.check_fit_file(native(), out, case.A, _frames(case), _camera_pixels(case), what="cpu dense on sparse")
    np.testing.assert_array_equal(again["value"], got["value"])
    np.testing.assert_array_equal(again["pixels"], got["pixels"])


def test_cli_fit_only_needs_an_output_file(dense, binary):  # noqa: F811
    d, case = dense
    r = _run_native(binary, ["--use_cpu", "--fit_only", "-o", str(d / "missing.h5"), *case.files])
    assert r.returncode != 0
    assert "fit_only needs solutions to project" in r.stderr and "missing.h5" in r.stderr, r.stderr


def test_cli_fit_stored_time_outside_time_range(dense, binary):  # noqa: F811
    d, case = dense
    out = str(d / "range.h5")
    r = _run_native(binary, BASE + ["-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run_native(binary, ["--use_cpu", "--fit_only", "-t", "0.05:1", "-o", out, *case.files])
    assert r.returncode != 0
    assert "Stored solution time 0 has no composite frame" in r.stderr, r.stderr
    with pytest.raises(RuntimeError):  # nothing was written
        native().read_dataset_f64(out, "fit/image")
    # with the whole range selected the same file is fitted
    r = _run_native(binary, ["--use_cpu", "--fit_only", "-o", out, *case.files])
    assert r.returncode == 0, r.stdout + r.stderr
    fb.check_fit_file(native(), out, case.A, _frames(case), _camera_pixels(case), what="after the refusal")
