"""The native driver's --profile lines (docs/FORMATS.md): the exact ordered key list of every line kind -- load
(with its nested rank0 object), frame by frame, a batched series' lead frame, its batched frames and its series line,
and the fit line. The lists are the ones the driver printed before its main() was split into units
(csrc/driver/profile_lines.cpp builds them now): tools and recorded profiles read these keys."""
import json

import pytest

from mpi_cuda_sartsolver_amd.io.fixtures import make_case
from test_native_driver import _run_native, binary  # noqa: F401  (the driver fixture and launcher)

LOAD = ["load", "load_s", "rtm_GB", "load_GBps", "setup_s", "read_s", "h2d_s", "wait_read_s", "wait_copy_s", "ranks",
        "parallel_read", "rank0", "rss_growth_MB_max", "shard_MB_max", "sparse", "rtm_format", "rtm_storage",
        "f16_flushed", "f16_flushed_fraction", "solver_path", "nnz", "driver"]
LOAD_FP64 = LOAD[:LOAD.index("nnz")] + ["fp64_semantics"] + LOAD[LOAD.index("nnz"):]
RANK0 = ["load_s", "setup_s", "read_s", "h2d_s", "blocks", "rows_per_block", "rows_per_read", "staging_MB",
         "rss_hwm_before_MB", "rss_hwm_after_malloc_MB", "rss_hwm_after_memset_MB", "rss_hwm_after_pinned_MB",
         "rss_hwm_after_setup_MB", "rss_hwm_after_first_read_MB", "rss_hwm_after_MB"]
FRAME = ["frame", "time", "status", "iterations", "convergence", "sweeps", "iters_per_s", "gflops", "rtm_GBps",
         "comm_ms", "comm_fallbacks", "ms", "solve_ms", "setup_ms", "iterate_ms", "finish_ms", "writer_ms",
         "queued_sweeps", "wait_frame_ms", "fused", "ranks", "comm", "device_comm", "driver"]
LEAD = ["frame", "time", "status", "iterations", "convergence", "ms", "batch", "warm_from", "warm_iter", "lead",
        "fused", "driver"]
BATCHED = ["frame", "time", "status", "iterations", "convergence", "ms", "batch", "warm_from", "warm_iter",
           "warm_live", "comm_fallbacks", "driver"]
SERIES = ["series", "frames", "sweeps", "queued_sweeps", "slot_util", "mean_iterations", "chained", "mean_warm_age",
          "series_ms", "chunk", "admit_cap", "src_age", "src_finished", "lead", "src_extrap", "drift", "stage_window",
          "restarts", "host_wait_ms", "host_stage_ms", "host_src_ms", "host_deliver_ms", "reader_ms", "sink_ms",
          "batch", "driver"]
FIT = ["fit", "frames", "groups", "fit_ms", "rtm_storage", "rtm_format", "ranks"]


def profile_lines(binary, tmp_path, args, files):  # noqa: F811
    """The parsed --profile lines of one driver run (every line must be one JSON object ending the line)."""
    prof = str(tmp_path / "p.jsonl")
    r = _run_native(binary, [*args, "--profile", prof, "-o", str(tmp_path / "o.h5"), *files])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    text = open(prof).read()
    assert text.endswith("}\n")
    return [json.loads(line) for line in text.splitlines()]


def _check_load(rec, keys, **values):
    assert list(rec) == keys, list(rec)
    assert list(rec["rank0"]) == RANK0, list(rec["rank0"])
    assert rec["load"] is True and rec["driver"] == "native"
    assert isinstance(rec["parallel_read"], bool) and isinstance(rec["sparse"], bool)
    for k, v in values.items():
        assert rec[k] == v, (k, rec[k])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return make_case(str(tmp_path_factory.mktemp("schema") / "case"), sparse_cameras=("cam_b",), laplacian=True,
                     nframes=3, saturate=0.05)


def test_cpu_frame_lines(tmp_path, binary, case):  # noqa: F811
    recs = profile_lines(binary, tmp_path, ["--use_cpu", "-m", "40", "-c", "1e-6"], case.files)
    assert len(recs) == 3
    for k, rec in enumerate(recs):
        assert list(rec) == FRAME, list(rec)
        assert rec["frame"] == k and rec["fused"] is False and rec["ranks"] == 1 and rec["device_comm"] == "none"
        assert rec["driver"] == "native" and rec["sweeps"] == rec["iterations"]


def test_cpu_sparse_load_line(tmp_path, binary, case):  # noqa: F811
    recs = profile_lines(binary, tmp_path, ["--use_cpu", "--rtm_format", "sparse", "-m", "40", "-c", "1e-6"], case.files)
    assert len(recs) == 4
    _check_load(recs[0], LOAD, rtm_format="sparse", rtm_storage="fp32", solver_path="cpu", ranks=1, f16_flushed=0)
    assert recs[0]["nnz"] > 0 and recs[0]["rank0"]["blocks"] == 0
    assert all(list(rec) == FRAME for rec in recs[1:])


def test_cpu_fit_line(tmp_path, binary, case):  # noqa: F811
    recs = profile_lines(binary, tmp_path, ["--use_cpu", "--fit", "-m", "40", "-c", "1e-6"], case.files)
    assert [list(rec) for rec in recs] == [FRAME] * 3 + [FIT]
    assert recs[-1] == dict(recs[-1], fit=True, frames=3, groups=1, rtm_storage="fp32", rtm_format="dense", ranks=1)


@pytest.fixture(scope="module")
def gpu_case(tmp_path_factory):
    return make_case(str(tmp_path_factory.mktemp("schema_gpu") / "case"), sparse_cameras=("cam_b",), laplacian=True,
                     nframes=4, saturate=0.05, nvoxel=2048, grid=(16, 16, 16), shapes=((24, 32), (20, 30)))


@pytest.mark.gpu
def test_gpu_load_and_frame_lines(tmp_path, binary, gpu_case):  # noqa: F811
    recs = profile_lines(binary, tmp_path, ["-m", "40", "-c", "1e-6"], gpu_case.files)
    assert len(recs) == 5
    _check_load(recs[0], LOAD, rtm_format="dense", rtm_storage="fp32", ranks=1, nnz=0, sparse=True)
    assert recs[0]["solver_path"] in ("fused", "two-pass") and recs[0]["rank0"]["blocks"] >= 1
    for rec in recs[1:]:
        assert list(rec) == FRAME, list(rec)
        assert isinstance(rec["fused"], bool) and rec["ranks"] == 1 and rec["driver"] == "native"


@pytest.mark.gpu
def test_gpu_batched_series_lines(tmp_path, binary, gpu_case):  # noqa: F811
    recs = profile_lines(binary, tmp_path, ["-m", "40", "-c", "1e-6", "--batch_frames", "2"], gpu_case.files)
    assert [list(rec) for rec in recs] == [LOAD, LEAD, BATCHED, BATCHED, BATCHED, SERIES]
    _check_load(recs[0], LOAD, rtm_format="dense", rtm_storage="fp32")
    assert recs[0]["solver_path"].startswith("multi-frame ")
    lead = recs[1]
    assert lead["frame"] == 0 and lead["lead"] is True and lead["warm_from"] == -1 and lead["warm_iter"] == -1
    assert [rec["frame"] for rec in recs[2:5]] == [1, 2, 3]  # written in time order
    assert all(rec["warm_live"] in (0, 1) and rec["warm_from"] >= 0 for rec in recs[2:5])
    series = recs[5]
    assert series["series"] is True and series["src_finished"] in (0, 1)
    assert series["lead"] in (0, 1) and series["driver"] == "native"


@pytest.mark.gpu
def test_gpu_fp64_load_line(tmp_path, binary, gpu_case):  # noqa: F811
    recs = profile_lines(binary, tmp_path, ["-m", "40", "-c", "1e-6", "--fp64"], gpu_case.files)
    assert len(recs) == 5
    _check_load(recs[0], LOAD_FP64, solver_path="fp64-two-pass", fp64_semantics="gpu", rtm_storage="fp32")
    assert all(list(rec) == FRAME for rec in recs[1:])
