"""--replicas in the native argument parser: the noise flags, what the run implies (16 batch columns, cold starts),
every refusal with its message, and the help text."""
import re

import pytest

from mpi_cuda_sartsolver_amd.ops import native

FILES = ["rtm.h5", "image.h5"]
REL = ["--noise_rel", "0.02"]


def _parse(*args):
    return native().parse_arguments([*args, *FILES])


def test_default_is_no_replicas():
    c = _parse()
    assert c.replicas == 0 and (c.noise_abs, c.noise_shot, c.noise_rel) == (0.0, 0.0, 0.0)
    assert c.noise_seed == 0 and c.replicas_keep is False and c.batch_frames == 1 and c.no_guess is False


@pytest.mark.parametrize("args", [
    ["--replicas", "7", "--noise_abs", "1e-3", "--noise_shot", "2.5e-4", "--noise_rel", "0.02", "--noise_seed",
     "18446744073709551615", "--replicas_keep"],
    ["--replicas_keep", "--noise_seed", "18446744073709551615", "--noise_rel", "0.02", "--noise_shot", "2.5e-4",
     "--noise_abs", "1e-3", "--replicas", "7"],
    ["--replicas=7", "--noise_abs=1e-3", "--noise_shot=2.5e-4", "--noise_rel=0.02",
     "--noise_seed=18446744073709551615", "--replicas_keep"],
])
def test_parses_in_any_order_and_form(args):
    c = _parse(*args)
    assert c.replicas == 7 and c.replicas_keep is True
    assert (c.noise_abs, c.noise_shot, c.noise_rel) == (1e-3, 2.5e-4, 0.02)
    assert c.noise_seed == 2 ** 64 - 1
    assert c.batch_frames == 16  # the default of 1 becomes the engine's narrowest batch
    assert c.no_guess is True    # every column cold-starts


def test_the_doubles_are_the_ones_repr_names():
    v = 0.1 + 0.2
    assert _parse("--replicas", "2", "--noise_abs", repr(v)).noise_abs == v


def test_larger_batches_are_kept_and_storages_combine():
    assert _parse("--replicas", "2", *REL, "--batch_frames", "32").batch_frames == 32
    assert _parse("--replicas", "2", *REL, "--batch_frames", "16").batch_frames == 16
    for extra in (["--rtm_bf16"], ["--rtm_f16"], ["--rtm_format", "sparse"], ["--rtm_format", "auto"], ["-L"],
                  ["--no_guess"], ["-l", "lap.h5"], ["-l", "lap.h5", "-b", "0.5"], ["--profile", "p.jsonl"]):
        c = _parse("--replicas", "2", *REL, *extra)
        assert c.replicas == 2 and c.no_guess and c.replicas_keep is False
    c = _parse("--replicas", "2", *REL, "-l", "lap.h5", "-b", "0.5")
    assert c.laplacian_file == "lap.h5" and c.beta_laplace == 0.5  # -l and -b keep their meaning
    assert _parse("--replicas", "2", *REL).laplacian_file == ""    # the Laplacian is optional


@pytest.mark.parametrize("n", ["2", "1024"])
def test_the_range_ends_are_accepted(n):
    assert _parse("--replicas", n, *REL).replicas == int(n)


@pytest.mark.parametrize("n", ["1", "0", "-3", "1025"])
def test_bad_counts(n):
    with pytest.raises(RuntimeError, match=re.escape(f"Argument replicas must be within 2 .. 1024, {n} given.")):
        _parse("--replicas=" + n, *REL)


@pytest.mark.parametrize("name", ["noise_abs", "noise_shot", "noise_rel"])
@pytest.mark.parametrize("value, shown", [("-1e-3", "-0.001"), ("nan", "nan"), ("inf", "inf")])
def test_negative_or_non_finite_noise(name, value, shown):
    with pytest.raises(RuntimeError, match=re.escape(f"Argument {name} must be finite and >= 0, {shown} given.")):
        _parse("--replicas", "4", "--noise_rel", "0.01", "--noise_abs", "0.01", "--noise_shot", "0.01",
               f"--{name}={value}")


@pytest.mark.parametrize("extra", [[], ["--noise_abs", "0"], ["--noise_abs", "0", "--noise_shot", "0", "--noise_rel",
                                                             "0"], ["--noise_seed", "3"]])
def test_needs_a_noise_term(extra):
    msg = "Argument replicas needs a noise term: one of noise_abs, noise_shot, noise_rel must be > 0."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse("--replicas", "4", *extra)


@pytest.mark.parametrize("args", [["--noise_abs", "1"], ["--noise_shot", "1"], ["--noise_rel", "1"],
                                  ["--noise_seed", "1"], ["--replicas_keep"]])
def test_the_noise_flags_need_replicas(args):
    msg = "Arguments noise_abs, noise_shot, noise_rel, noise_seed and replicas_keep need replicas."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse(*args)


@pytest.mark.parametrize("seed", ["-1", "18446744073709551616", "1.5", "abc", ""])
def test_bad_seeds(seed):
    with pytest.raises(RuntimeError, match="as an unsigned 64-bit integer for --noise_seed"):
        _parse("--replicas", "4", *REL, "--noise_seed=" + seed)


@pytest.mark.parametrize("extra", [["--use_cpu"], ["--fp64"], ["--partition_voxels"]])
def test_batched_gpu_row_shards_only(extra):
    msg = "Argument replicas applies to the batched GPU solver with pixel-row shards only."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse("--replicas", "4", *REL, *extra)


@pytest.mark.parametrize("extra", [["--resume"], ["--fit"], ["--fit_only"],
                                   ["-l", "lap.h5", "--beta_scan", "0,1,2"]])
def test_writes_its_own_output(extra):
    msg = "Argument replicas writes its own output: it cannot be combined with resume, fit, fit_only or beta_scan."
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _parse("--replicas", "4", *REL, *extra)


def test_usage_names_the_flags_between_beta_scan_and_profile():
    u = native().usage()
    flags = ["--replicas N", "--noise_abs", "--noise_shot", "--noise_rel", "--noise_seed", "--replicas_keep"]
    pos = [u.index("  " + f) for f in flags]
    assert pos == sorted(pos) and u.index("  --beta_scan") < pos[0] and pos[-1] < u.index("  --profile")
    assert "/uncertainty" in u and "sigma^2 = A^2 + S g + (R g)^2" in u
