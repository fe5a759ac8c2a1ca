"""--holdout in the native argument parser: the fold count or `cameras`, the seed and the ladder in either form, what
the run implies (16 batch columns, cold starts), what it combines with, every refusal with its message, and the help
text. The refusals that need the inputs (fewer than two cameras with `cameras`, 2^32 pixels and more) are the driver's:
the first is in tests/test_cli_holdout.py, the second has no fixture of that size."""
import re

import pytest

from mpi_cuda_sartsolver_amd.ops import native

FILES = ["rtm.h5", "image.h5"]
ROWS = "Argument holdout applies to the batched GPU solver with pixel-row shards only."
OWN = ("Argument holdout writes its own output: it cannot be combined with resume, fit, fit_only, beta_scan, replicas or "
       "phantom.")
RANGE = "Argument holdout must be cameras or a number of folds within 2 .. 32, "


def _parse(*args):
    return native().parse_arguments([*args, *FILES])


def test_default_is_no_holdout():
    c = _parse()
    assert c.holdout == 0 and c.holdout_cameras is False and c.holdout_seed == 0 and list(c.holdout_betas) == []
    assert c.batch_frames == 1 and c.no_guess is False


@pytest.mark.parametrize("args", [["--holdout", "4"], ["--holdout=4"]])
def test_parses_a_fold_count_in_either_form(args):
    c = _parse(*args)
    assert c.holdout == 4 and c.holdout_cameras is False and c.holdout_seed == 0 and list(c.holdout_betas) == []
    assert c.batch_frames == 16  # the default of 1 becomes the engine's narrowest batch
    assert c.no_guess is True    # every column cold-starts


@pytest.mark.parametrize("args", [["--holdout", "cameras"], ["--holdout=cameras"]])
def test_parses_cameras_in_either_form(args):
    c = _parse(*args)
    assert c.holdout_cameras is True and c.holdout == 0  # K is the number of cameras, known with the inputs
    assert c.batch_frames == 16 and c.no_guess is True


@pytest.mark.parametrize("k", [2, 32])
def test_fold_count_limits(k):
    assert _parse("--holdout", str(k)).holdout == k


@pytest.mark.parametrize("k", ["0", "1", "33", "-4"])
def test_fold_count_out_of_range(k):
    with pytest.raises(RuntimeError, match=re.escape(RANGE + k + " given.")):
        _parse("--holdout=" + k)


@pytest.mark.parametrize("text", ["four", "4.5", "camera", ""])
def test_fold_count_must_be_a_number_or_cameras(text):
    with pytest.raises(RuntimeError, match=re.escape(f"Failed to parse '{text}' as an integer for --holdout.")):
        _parse("--holdout=" + text)


@pytest.mark.parametrize("args", [["--holdout_seed", "18446744073709551615"], ["--holdout_seed=18446744073709551615"]])
def test_seed_is_64_bits_in_either_form(args):
    assert _parse("--holdout", "4", *args).holdout_seed == 2 ** 64 - 1


@pytest.mark.parametrize("text", ["-1", "+1", "1.5", "18446744073709551616", "x"])
def test_seed_parses_like_noise_seed(text):
    msg = f"Failed to parse '{text}' as an unsigned 64-bit integer for --holdout_seed."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse("--holdout", "4", "--holdout_seed=" + text)


def test_seed_needs_holdout_and_pixel_folds():
    with pytest.raises(RuntimeError, match=re.escape("Arguments holdout_seed and holdout_betas need holdout.")):
        _parse("--holdout_seed", "3")
    msg = "Argument holdout_seed applies to pixel folds: it cannot be combined with holdout cameras."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse("--holdout", "cameras", "--holdout_seed", "3")


@pytest.mark.parametrize("args", [["--holdout_betas", "0,1e-3,1e-2"], ["--holdout_betas=0, 1e-3 ,1e-2"]])
def test_ladder_in_either_form(args):
    c = _parse("--holdout", "4", "-l", "lap.h5", *args)
    assert list(c.holdout_betas) == [0.0, 1e-3, 1e-2] and list(c.beta_scan) == []
    c = _parse("--holdout", "cameras", "-l", "lap.h5", *args)
    assert list(c.holdout_betas) == [0.0, 1e-3, 1e-2] and c.holdout_cameras


@pytest.mark.parametrize("text", ["1,2", "3,2,1", "0,1,1", "-1,0,1", "0,1,nan", "0,,1", "a,b,c",
                                  ",".join(str(i) for i in range(65))])
def test_ladder_follows_the_scan_rules(text):
    msg = "Argument holdout_betas must list 3 to 64 increasing values >= 0, " + text + " given."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse("--holdout", "4", "-l", "lap.h5", "--holdout_betas=" + text)


def test_the_scan_keeps_its_own_message():
    with pytest.raises(RuntimeError, match=re.escape("Argument beta_scan must list 3 to 64 increasing values >= 0, 1,2")):
        _parse("-l", "lap.h5", "--beta_scan", "1,2")


def test_ladder_needs_a_laplacian_and_holdout():
    with pytest.raises(RuntimeError, match=re.escape("Argument holdout_betas needs a laplacian_file.")):
        _parse("--holdout", "4", "--holdout_betas", "0,1,2")
    with pytest.raises(RuntimeError, match=re.escape("Arguments holdout_seed and holdout_betas need holdout.")):
        _parse("-l", "lap.h5", "--holdout_betas", "0,1,2")


def test_larger_batches_are_kept_and_one_is_raised():
    assert _parse("--holdout", "4", "--batch_frames", "32").batch_frames == 32
    assert _parse("--batch_frames", "64", "--holdout", "cameras").batch_frames == 64
    assert _parse("--holdout", "4", "--batch_frames", "1").batch_frames == 16


@pytest.mark.parametrize("extra", [["--rtm_bf16"], ["--rtm_f16"], ["--rtm_format", "sparse"], ["-L"], ["-l", "lap.h5"],
                                   ["-l", "lap.h5", "-b", "0.5"], ["--no_guess"], ["--profile", "p.jsonl"], ["-m", "60"]])
def test_what_it_combines_with(extra):
    c = _parse("--holdout", "4", *extra)
    assert c.holdout == 4 and c.no_guess
    if "-b" in extra:
        assert c.beta_laplace == 0.5 and c.laplacian_file == "lap.h5"


@pytest.mark.parametrize("mode", ["4", "cameras"])
@pytest.mark.parametrize("extra", [["--use_cpu"], ["--fp64"], ["--partition_voxels"]])
def test_batched_gpu_row_shards_only(extra, mode):
    with pytest.raises(RuntimeError, match=re.escape(ROWS)):
        _parse("--holdout", mode, *extra)


@pytest.mark.parametrize("extra", [["--resume"], ["--fit"], ["--fit_only"], ["-l", "lap.h5", "--beta_scan", "0,1,2"],
                                   ["--replicas", "4", "--noise_rel", "0.02"], ["--phantom", "t.h5"]])
def test_writes_its_own_output(extra):
    with pytest.raises(RuntimeError, match=re.escape(OWN)):
        _parse("--holdout", "4", *extra)


def test_needs_a_value():
    with pytest.raises(RuntimeError, match=re.escape("Too few arguments for --holdout.")):
        native().parse_arguments(["--holdout"])


def test_usage_names_the_flags_between_phantom_and_profile():
    u = native().usage()
    pos = u.index("  --holdout K|cameras")
    assert u.index("  --phantom FILE") < pos < u.index("  --holdout_seed S") < u.index("  --holdout_betas B0,B1,...")
    assert u.index("  --holdout_betas") < u.index("  --profile")
    text = " ".join(u[pos: u.index("  --holdout_seed")].split())
    assert "/holdout group" in text and "2 to 32" in text and "at least two cameras" in text
    for flag in ("--use_cpu", "--fp64", "--partition_voxels", "--resume", "--fit,", "--fit_only", "--beta_scan",
                 "--replicas", "--phantom"):
        assert flag in text[text.index("Not with"):], flag
