"""--rtm_f16_fused in the native config parser (csrc/native/config.cpp): the opt-in to the fused single-pass sweep on
row-scaled f16 shards. A plain flag that needs --rtm_f16, documented right after it."""
import pytest

from mpi_cuda_sartsolver_amd.ops import native


@pytest.fixture(scope="module")
def n():
    return native()


def test_rtm_f16_fused_parses(n):
    c = n.parse_arguments(["--rtm_f16", "a.h5", "b.h5"])
    assert c.rtm_f16 and not c.rtm_f16_fused
    c = n.parse_arguments(["--rtm_f16", "--rtm_f16_fused", "a.h5", "b.h5"])
    assert c.rtm_f16 and c.rtm_f16_fused and not c.rtm_bf16 and not c.two_pass
    assert c.input_files == ["a.h5", "b.h5"]
    c = n.parse_arguments(["--rtm_f16_fused", "--rtm_f16", "a", "b"])  # any order
    assert c.rtm_f16 and c.rtm_f16_fused


def test_rtm_f16_fused_with_two_pass_keeps_all_three(n):
    c = n.parse_arguments(["--rtm_f16", "--rtm_f16_fused", "--two_pass", "a", "b"])
    assert c.rtm_f16 and c.rtm_f16_fused and c.two_pass


def test_rtm_f16_fused_is_ignored_by_batches_not_refused(n):
    c = n.parse_arguments(["--rtm_f16", "--rtm_f16_fused", "--batch_frames", "16", "a", "b"])
    assert c.rtm_f16_fused and c.batch_frames == 16


@pytest.mark.parametrize("argv,msg", [
    (["--rtm_f16_fused", "a", "b"], "Argument rtm_f16_fused needs rtm_f16."),
    (["--rtm_bf16", "--rtm_f16_fused", "a", "b"], "Argument rtm_f16_fused needs rtm_f16."),
    (["--rtm_f16", "--rtm_f16_fused=1", "a", "b"], "does not take a value"),
    (["--rtm_f16_fused=1", "a", "b"], "does not take a value"),
])
def test_rtm_f16_fused_validation(n, argv, msg):
    with pytest.raises(RuntimeError, match=msg):
        n.parse_arguments(argv)


def test_usage_documents_it_between_rtm_f16_and_rtm_format(n):
    u = n.usage()
    assert "--rtm_f16_fused" in u
    assert u.index("--rtm_f16") < u.index("--rtm_f16_fused") < u.index("--rtm_format")
    assert u.index("--rtm_f16") != u.index("--rtm_f16_fused")  # (--rtm_f16's own line comes first)
