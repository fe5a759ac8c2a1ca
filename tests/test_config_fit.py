"""--fit / --fit_only in the native argument parser: parsing, the help text, what --fit_only refuses, and that --fit
combines with every other option."""
import pytest

from mpi_cuda_sartsolver_amd.ops import native

FILES = ["rtm.h5", "image.h5"]


def _parse(*args):
    return native().parse_arguments([*args, *FILES])


def test_fit_flags_default_off_and_parse():
    c = _parse()
    assert c.fit is False and c.fit_only is False
    c = _parse("--fit")
    assert c.fit is True and c.fit_only is False
    c = _parse("--fit_only", "-o", "x.h5")
    assert c.fit_only is True and c.fit is False and c.output_file == "x.h5"
    c = _parse("--fit", "--fit_only")
    assert c.fit and c.fit_only


def test_fit_flags_take_no_value():
    for flag in ("--fit", "--fit_only"):
        with pytest.raises(RuntimeError, match="does not take a value"):
            _parse(flag + "=1")


def test_usage_names_both_flags():
    u = native().usage()
    assert "--fit " in u and "--fit_only" in u and "/fit group" in u


@pytest.mark.parametrize("extra, word", [(["--resume"], "resume"), (["--batch_frames", "16"], "batch_frames"),
                                         (["--fp64"], "fp64")])
def test_fit_only_refusals(extra, word):
    with pytest.raises(RuntimeError, match=r"Argument fit_only .*" + word):
        _parse("--fit_only", *extra)
    # the same options are fine with --fit
    c = _parse("--fit", *extra)
    assert c.fit


@pytest.mark.parametrize("extra", [
    [], ["--two_pass"], ["--rtm_bf16"], ["--rtm_f16"], ["--rtm_f16", "--rtm_f16_fused"], ["--rtm_format", "sparse"],
    ["--rtm_format", "dense"], ["--batch_frames", "64"], ["--fp64"], ["--fp64", "--fp64_semantics", "cpu"],
    ["--partition_voxels"], ["--use_cpu"], ["--use_cpu", "--rtm_format", "sparse"], ["--resume"], ["--no_guess"],
    ["-L"], ["--parallel_read"], ["--profile", "p.jsonl"], ["-t", "0:1"], ["-l", "lap.h5", "-b", "0.1"],
    ["-m", "10", "-c", "1e-3", "-R", "0.5", "-d", "1e-5", "-r", "1e-5", "-w", "10", "-n", "no_reflections"],
    ["--max_cached_frames", "3", "--max_cached_solutions", "3"],
], ids=lambda e: " ".join(e) or "defaults")
def test_fit_combines_with_every_option(extra):
    c = _parse("--fit", *extra)
    assert c.fit and not c.fit_only
    without = _parse(*extra)
    for name in ("two_pass", "rtm_bf16", "rtm_f16", "rtm_f16_fused", "rtm_format", "batch_frames", "fp64",
                 "fp64_semantics", "partition_voxels", "use_cpu", "resume", "no_guess", "logarithmic", "parallel_read",
                 "profile_file", "time_range", "max_iterations"):
        assert getattr(c, name) == getattr(without, name), name


@pytest.mark.parametrize("extra", [[], ["--rtm_bf16"], ["--rtm_f16"], ["--rtm_format", "sparse"], ["--partition_voxels"],
                                   ["--use_cpu"], ["--use_cpu", "--rtm_format", "sparse"], ["--two_pass"]],
                         ids=lambda e: " ".join(e) or "defaults")
def test_fit_only_combines_with_the_storages(extra):
    assert _parse("--fit_only", *extra).fit_only
