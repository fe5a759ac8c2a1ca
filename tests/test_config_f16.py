"""--rtm_f16 in the native config parser (csrc/native/config.cpp): parsed, documented, exclusive with --rtm_bf16 and
refused exactly where --rtm_bf16 is; and the f16 storage path of the multi-frame planner (one planner, variant
tables: csrc/engine/mf_plan.cpp)."""
import pytest

from mpi_cuda_sartsolver_amd.ops import native


@pytest.fixture(scope="module")
def n():
    return native()


def test_rtm_f16_parses(n):
    c = n.parse_arguments(["a.h5", "b.h5"])
    assert not c.rtm_f16 and not c.rtm_bf16
    c = n.parse_arguments(["--rtm_f16", "a.h5", "b.h5"])
    assert c.rtm_f16 and not c.rtm_bf16 and c.input_files == ["a.h5", "b.h5"]
    c = n.parse_arguments(["--rtm_f16", "--batch_frames", "16", "--two_pass", "a", "b"])
    assert c.rtm_f16 and c.batch_frames == 16 and c.two_pass
    assert not n.parse_arguments(["--rtm_bf16", "a", "b"]).rtm_f16


def test_usage_names_rtm_f16(n):
    u = n.usage()
    assert "--rtm_f16" in u and u.index("--rtm_bf16") < u.index("--rtm_f16") < u.index("--rtm_format")


@pytest.mark.parametrize("argv,msg", [
    (["--rtm_f16", "--rtm_bf16", "a", "b"], "rtm_f16 and rtm_bf16 are exclusive"),
    (["--rtm_bf16", "--rtm_f16", "a", "b"], "rtm_f16 and rtm_bf16 are exclusive"),
    (["--rtm_f16", "--use_cpu", "a", "b"], "rtm_f16 applies to the GPU solvers with pixel-row shards"),
    (["--rtm_f16", "--partition_voxels", "a", "b"], "rtm_f16 applies to the GPU solvers with pixel-row shards"),
    (["--rtm_f16", "--rtm_format", "sparse", "a", "b"], "rtm_format sparse applies to fp32"),
    (["--rtm_f16=1", "a", "b"], "does not take a value"),
])
def test_rtm_f16_validation(n, argv, msg):
    with pytest.raises(RuntimeError, match=msg):
        n.parse_arguments(argv)


# ---------------------------------------------------------------------------- the planner's f16 storage path ("s16")


@pytest.fixture(scope="module")
def k():
    from mpi_cuda_sartsolver_amd.ops import hip

    return hip()


def _strip(d):
    return {x: v for x, v in d.items() if x not in ("path", "nsplit", "cps", "rps", "grid", "vox_align")}


@pytest.mark.parametrize("nf", [16, 32, 64, 128])
@pytest.mark.parametrize("ld,rows", [(1024, 512), (1088, 1000), (4096, 2048), (65536, 65536)])
def test_s16_plans_are_the_bf16_storage_defaults(k, monkeypatch, nf, ld, rows):
    for v in ("SART_MF_DEPTH", "SART_MF_B16_FWD", "SART_MF_B16_VT", "SART_MF_XEARLY", "SART_MF_WEARLY",
              "SART_MF_FWD_BLOCKS", "SART_MF_BP_BLOCKS"):
        monkeypatch.delenv(v, raising=False)
    pad = (rows + 63) // 64 * 64
    fs, fb = k.mf_plan_forward("s16", nf, ld, pad), k.mf_plan_forward("b16", nf, ld, pad)
    assert fs["path"] == "s16" and _strip(fs) == _strip(fb)
    assert (fs["nsplit"], fs["cps"], fs["grid"]) == (fb["nsplit"], fb["cps"], fb["grid"])
    bs, bb = k.mf_plan_backproject("s16", nf, ld, rows), k.mf_plan_backproject("b16", nf, ld, rows)
    assert bs["path"] == "s16" and _strip(bs) == _strip(bb)
    assert (bs["nsplit"], bs["rps"], bs["vox_align"], bs["grid"]) == (bb["nsplit"], bb["rps"], bb["vox_align"], bb["grid"])
    # every default plan has its kernel in the table
    assert _strip(fs) in [_strip({x: v for x, v in d.items() if x != "env"}) for d in k.mf_variants("s16", nf, True)]
    assert _strip(bs) in [_strip({x: v for x, v in d.items() if x != "env"}) for d in k.mf_variants("s16", nf, False)]


def test_s16_lists_only_the_default_keys(k):
    assert [len(k.mf_variants("s16", nf, True)) for nf in (16, 32, 64, 128)] == [1, 1, 1, 1]
    assert [len(k.mf_variants("s16", nf, False)) for nf in (16, 32, 64, 128)] == [2, 2, 2, 1]


def test_s16_has_no_knobs_of_its_own(k, monkeypatch):
    """A knob that moves the bf16-storage key away from the default asks for a kernel the f16 tables do not hold: the
    planner throws (nothing falls back), naming the knob."""
    monkeypatch.setenv("SART_MF_DEPTH", "2")
    with pytest.raises(RuntimeError, match="s16 path: no kernel for SART_MF_DEPTH=2"):
        k.mf_plan_forward("s16", 64, 2048, 1024)
    with pytest.raises(RuntimeError, match="s16 path: no kernel for SART_MF_DEPTH=2"):
        k.mf_plan_backproject("s16", 64, 2048, 1000)
    assert k.mf_plan_forward("b16", 64, 2048, 1024)["depth"] == 2  # bf16 storage keeps its A/B variants


def test_s16_needs_64_row_padding(k):
    with pytest.raises(RuntimeError, match="padded rows must be a multiple of 64"):
        k.mf_plan_forward("s16", 16, 1024, 96)
