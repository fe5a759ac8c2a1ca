"""--beta_scan in the native argument parser: the ladder, what it implies (16 batch columns, cold starts), every refusal
with its message, and the help text."""
import re

import pytest

from mpi_cuda_sartsolver_amd.ops import native

FILES = ["rtm.h5", "image.h5"]
LAP = ["-l", "lap.h5"]


def _parse(*args):
    return native().parse_arguments([*args, *FILES])


def test_default_is_no_scan():
    c = _parse()
    assert list(c.beta_scan) == [] and c.batch_frames == 1 and c.no_guess is False


@pytest.mark.parametrize("args", [["--beta_scan", "0,1e-3,1e-2"], ["--beta_scan=0,1e-3,1e-2"],
                                  ["--beta_scan", " 0, 1e-3 ,1e-2"]])
def test_parses_the_ladder(args):
    c = _parse(*LAP, *args)
    assert list(c.beta_scan) == [0.0, 1e-3, 1e-2]
    assert c.batch_frames == 16  # the default of 1 becomes the engine's narrowest batch
    assert c.no_guess is True    # every column cold-starts
    assert c.beta_laplace == 0.02  # -b is left alone: it names the fallback entry


def test_larger_batches_are_kept_and_storages_combine():
    assert _parse(*LAP, "--beta_scan", "0,1,2", "--batch_frames", "64").batch_frames == 64
    assert _parse(*LAP, "--beta_scan", "0,1,2", "--batch_frames", "16").batch_frames == 16
    for extra in (["--rtm_bf16"], ["--rtm_f16"], ["--rtm_format", "sparse"], ["--rtm_format", "auto"], ["-L"],
                  ["--no_guess"], ["-b", "0.5"], ["--profile", "p.jsonl"]):
        c = _parse(*LAP, "--beta_scan", "0,1,2", *extra)
        assert list(c.beta_scan) == [0.0, 1.0, 2.0] and c.no_guess


def test_64_values_are_accepted():
    text = ",".join(str(i) for i in range(64))
    assert len(_parse(*LAP, "--beta_scan", text).beta_scan) == 64


@pytest.mark.parametrize("text", [
    "1,2",                                 # too few
    ",".join(str(i) for i in range(65)),   # too many
    "-1,0,1",                              # negative
    "0,2,1",                               # not increasing
    "0,1,1",                               # not strictly increasing
    "0,abc,1", "0,,1", "", "0,1,2,",       # malformed
    "0,1,inf", "0,1,nan",                  # not finite
])
def test_bad_ladders(text):
    msg = f"Argument beta_scan must list 3 to 64 increasing values >= 0, {text} given."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse(*LAP, "--beta_scan=" + text)


def test_needs_a_laplacian():
    with pytest.raises(RuntimeError, match=re.escape("Argument beta_scan needs a laplacian_file.")):
        _parse("--beta_scan", "0,1,2")


@pytest.mark.parametrize("extra", [["--use_cpu"], ["--fp64"], ["--partition_voxels"]])
def test_batched_gpu_row_shards_only(extra):
    msg = "Argument beta_scan applies to the batched GPU solver with pixel-row shards only."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse(*LAP, "--beta_scan", "0,1,2", *extra)


@pytest.mark.parametrize("extra", [["--resume"], ["--fit"], ["--fit_only"]])
def test_writes_its_own_output(extra):
    msg = "Argument beta_scan writes its own output: it cannot be combined with resume, fit or fit_only."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse(*LAP, "--beta_scan", "0,1,2", *extra)


def test_usage_names_the_flag():
    u = native().usage()
    assert "--beta_scan" in u and "/beta_scan" in u
