"""--phantom in the native argument parser: what the run implies (16 batch columns, cold starts), what it combines with
(--replicas and the noise flags, the storages, -l / -b, -L), every refusal with its message, and the help text."""
import re

import pytest

from mpi_cuda_sartsolver_amd.ops import native

FILES = ["rtm.h5", "image.h5"]
REP = ["--replicas", "4", "--noise_rel", "0.02"]
ROWS = "Argument phantom applies to the batched GPU solver with pixel-row shards only."
OWN = "Argument phantom writes its own output: it cannot be combined with resume, fit, fit_only or beta_scan."


def _parse(*args):
    return native().parse_arguments([*args, *FILES])


def test_default_is_no_phantom():
    c = _parse()
    assert c.phantom_file == "" and c.batch_frames == 1 and c.no_guess is False


@pytest.mark.parametrize("args", [["--phantom", "truth.h5"], ["--phantom=truth.h5"]])
def test_parses_in_either_form(args):
    c = _parse(*args)
    assert c.phantom_file == "truth.h5" and c.replicas == 0
    assert c.batch_frames == 16  # the default of 1 becomes the engine's narrowest batch
    assert c.no_guess is True    # every column cold-starts


def test_larger_batches_are_kept():
    assert _parse("--phantom", "t.h5", "--batch_frames", "32").batch_frames == 32
    assert _parse("--batch_frames", "16", "--phantom", "t.h5").batch_frames == 16


@pytest.mark.parametrize("extra", [["--rtm_bf16"], ["--rtm_f16"], ["--rtm_format", "sparse"], ["--rtm_format", "auto"],
                                   ["-L"], ["--logarithmic"], ["-l", "lap.h5"], ["-l", "lap.h5", "-b", "0.5"],
                                   ["--no_guess"], ["--profile", "p.jsonl"], ["-t", "0:1"], ["-m", "60"]])
def test_what_it_combines_with(extra):
    c = _parse("--phantom", "t.h5", *extra)
    assert c.phantom_file == "t.h5" and c.no_guess and c.replicas == 0


def test_l_and_b_keep_their_meaning():
    c = _parse("--phantom", "t.h5", "-l", "lap.h5", "-b", "0.5")
    assert c.laplacian_file == "lap.h5" and c.beta_laplace == 0.5
    assert _parse("--phantom", "t.h5").laplacian_file == ""  # the Laplacian is optional


@pytest.mark.parametrize("order", [0, 1])
def test_replicas_and_the_noise_flags_combine(order):
    rep = ["--replicas", "7", "--noise_abs", "1e-3", "--noise_shot", "2.5e-4", "--noise_rel", "0.02", "--noise_seed", "9",
           "--replicas_keep"]
    ph = ["--phantom", "t.h5"]
    c = _parse(*(rep + ph if order else ph + rep))
    assert c.phantom_file == "t.h5" and c.replicas == 7 and c.replicas_keep is True and c.noise_seed == 9
    assert (c.noise_abs, c.noise_shot, c.noise_rel) == (1e-3, 2.5e-4, 0.02) and c.batch_frames == 16


def test_the_replicas_rules_still_hold_with_a_phantom():
    with pytest.raises(RuntimeError, match=re.escape("Argument replicas needs a noise term")):
        _parse("--phantom", "t.h5", "--replicas", "4")
    with pytest.raises(RuntimeError, match=re.escape("need replicas.")):
        _parse("--phantom", "t.h5", "--noise_rel", "0.1")


@pytest.mark.parametrize("rep", [[], REP], ids=["alone", "replicas"])
@pytest.mark.parametrize("extra", [["--use_cpu"], ["--fp64"], ["--partition_voxels"], ["--batch_frames", "1"],
                                   ["--batch_frames=1"]])
def test_batched_gpu_row_shards_only(extra, rep):
    # with --replicas its own refusal, the same words, may come first
    first = ROWS.replace("phantom", "replicas") if rep and "--batch_frames" not in extra[0] else ROWS
    with pytest.raises(RuntimeError, match=re.escape(first)):
        _parse("--phantom", "t.h5", *rep, *extra)


@pytest.mark.parametrize("extra", [["--resume"], ["--fit"], ["--fit_only"], ["-l", "lap.h5", "--beta_scan", "0,1,2"]])
def test_writes_its_own_output(extra):
    with pytest.raises(RuntimeError, match=re.escape(OWN)):
        _parse("--phantom", "t.h5", *extra)


def test_needs_a_file_name():
    with pytest.raises(RuntimeError, match=re.escape("Argument phantom needs a file name.")):
        _parse("--phantom=")
    with pytest.raises(RuntimeError, match=re.escape("Too few arguments for --phantom.")):
        native().parse_arguments(["--phantom"])


def test_usage_names_the_flag_between_replicas_keep_and_profile():
    u = native().usage()
    pos = u.index("  --phantom FILE")
    assert u.index("  --replicas_keep") < pos < u.index("  --profile")
    text = " ".join(u[pos: u.index("  --profile")].split())
    assert "/phantom group" in text and "/phantom/value" in text
    assert "frames and -t / --time_range are not used" in text  # the images only fix the cameras and pixels
    for flag in ("--use_cpu", "--batch_frames 1", "--fp64", "--partition_voxels", "--resume", "--fit,", "--fit_only",
                 "--beta_scan"):
        assert flag in text[text.index("Not with"):], flag
