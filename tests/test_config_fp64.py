"""--fp64 / --fp64_semantics in the native config parser (csrc/native/config.cpp): parsed, documented, defaulted, and
refused with every option the double-precision engine does not serve."""
import pytest

from mpi_cuda_sartsolver_amd.ops import native


@pytest.fixture(scope="module")
def n():
    return native()


def test_fp64_defaults(n):
    c = n.parse_arguments(["a.h5", "b.h5"])
    assert c.fp64 is False and c.fp64_semantics == "gpu"


def test_fp64_parses(n):
    c = n.parse_arguments(["--fp64", "a.h5", "b.h5"])
    assert c.fp64 and c.fp64_semantics == "gpu" and c.input_files == ["a.h5", "b.h5"]
    assert not (c.use_cpu or c.rtm_bf16 or c.rtm_f16 or c.two_pass) and c.batch_frames == 1 and c.rtm_format == "auto"
    c = n.parse_arguments(["--fp64", "--fp64_semantics", "cpu", "-L", "a", "b"])
    assert c.fp64 and c.fp64_semantics == "cpu" and c.logarithmic
    c = n.parse_arguments(["--fp64_semantics=gpu", "--fp64", "a", "b"])  # any order, --name=value
    assert c.fp64 and c.fp64_semantics == "gpu"
    for ok in (["--no_guess"], ["--resume"], ["--rtm_format", "dense"], ["--rtm_format", "auto"], ["--two_pass"],
               ["--batch_frames", "1"], ["--profile", "p.jsonl"]):
        assert n.parse_arguments(["--fp64", *ok, "a", "b"]).fp64


def test_usage_names_both_flags(n):
    u = n.usage()
    assert "--fp64 " in u and "--fp64_semantics" in u and "gpu | cpu" in u
    assert u.index("--rtm_format") < u.index("--fp64 ") < u.index("--fp64_semantics") < u.index("--profile")


@pytest.mark.parametrize("argv,msg", [
    (["--fp64", "--use_cpu", "a", "b"], "fp64 applies to the GPU solver"),
    (["--fp64", "--batch_frames", "16", "a", "b"], "fp64 applies to the single-frame GPU solver only"),
    (["--fp64", "--batch_frames=2", "a", "b"], "fp64 applies to the single-frame GPU solver only"),
    (["--fp64", "--partition_voxels", "a", "b"], "fp64 applies to pixel-row shards only"),
    (["--fp64", "--rtm_bf16", "a", "b"], "fp64 applies to fp32 RTM storage only"),
    (["--rtm_f16", "--fp64", "a", "b"], "fp64 applies to fp32 RTM storage only"),
    (["--fp64", "--rtm_format", "sparse", "a", "b"], "fp64 applies to dense shards only"),
    (["--fp64_semantics", "cpu", "a", "b"], "fp64_semantics needs fp64"),
    (["--fp64_semantics", "gpu", "a", "b"], "fp64_semantics needs fp64"),
    (["--fp64_semantics", "cpu", "--use_cpu", "a", "b"], "fp64_semantics needs fp64"),
    (["--fp64", "--fp64_semantics", "fp32", "a", "b"], "fp64_semantics must be gpu or cpu, fp32 given"),
    (["--fp64", "--fp64_semantics"], "Too few arguments for --fp64_semantics"),
    (["--fp64=1", "a", "b"], "does not take a value"),
])
def test_fp64_refusals(n, argv, msg):
    with pytest.raises(RuntimeError, match=msg):
        n.parse_arguments(argv)
