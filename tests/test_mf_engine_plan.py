"""The multi-frame engine's plan (csrc/engine/mf_engine_plan.cpp) on the CPU: paths, batch clamp, operand layout,
queue capacities, chunk length, chain policy, voxel chunks and the seventeen environment variables, against values
written out here from the rules in that file's header.

Chunk lengths are t = bytes / 5e12 + 52e-6, chunk = min(32, max(min(check_interval, 4), ceil(1.5e-3 / t))):
fp32 64 x 1024: bytes 524288, t 5.2105e-5, 28.79 -> 29. bf16 16384^2: bytes 1.0737e9, t 2.6675e-4, 5.62 -> 6.
fp32 65536^2: t 6.9e-3, 0.22 -> 1, raised to min(check_interval, 4). Sparse with 10^6 entries: bytes 1.6e7,
t 5.52e-5, 27.17 -> 28 (the ceiling of the rule; a figure of 27 for this case would be the floor)."""
import pytest

from mpi_cuda_sartsolver_amd.ops import hip

ENGINE_KNOBS = ("SART_MF_X3", "SART_MF_BWD16", "SART_MF_FWD16", "SART_MF_XBLK", "SART_MF_LAST_BWD", "SART_MF_CHUNK",
                "SART_MF_GRAPH", "SART_MF_ADMIT_CAP", "SART_MF_SRC_AGE", "SART_MF_SRC_FINISHED", "SART_MF_LEAD",
                "SART_MF_SRC_EXTRAP", "SART_MF_DRIFT", "SART_MF_STAGE_WINDOW", "SART_MF_CHUNKS", "SART_FAULT_NAN",
                "SART_MF_SPARSE_PW")
LAUNCH_KNOBS = ("SART_MF_DEPTH", "SART_MF_ROWS", "SART_MF_VOX", "SART_MF_NT", "SART_MF_B16_FWD", "SART_MF_B16_VT",
                "SART_MF_X3_FWD", "SART_MF_X3_DEPTH", "SART_MF_X3_VT", "SART_MF_XEARLY", "SART_MF_WEARLY",
                "SART_MF_H16", "SART_MF_H16_FDEPTH", "SART_MF_FWD_BLOCKS", "SART_MF_BP_BLOCKS")
STORAGES = ("fp32", "bf16", "f16s", "sparse")
WIDTH = {1: 16, 16: 16, 17: 32, 32: 32, 64: 64, 65: 128, 128: 128, 500: 128}


@pytest.fixture
def k(monkeypatch):
    for name in ENGINE_KNOBS + LAUNCH_KNOBS:
        monkeypatch.delenv(name, raising=False)
    return hip()


def plan(k, storage="fp32", frames=64, nrows=700, nrows_pad=704, ld=1024, nnz=0, ranks=1, mf_split_a=-1,
         check_interval=16):
    sparse = storage == "sparse"
    name = {"fp32": "f32", "sparse": "f32", "bf16": "bf16", "f16s": "f16"}[storage]
    return k.mf_engine_plan(name, sparse, nnz, frames, nrows, nrows_pad, ld, ranks=ranks, mf_split_a=mf_split_a,
                            check_interval=check_interval)


@pytest.mark.parametrize("frames", sorted(WIDTH))
@pytest.mark.parametrize("storage", STORAGES)
def test_defaults(k, storage, frames):
    p = plan(k, storage, frames)
    nf = WIDTH[frames]  # no default path clamps 128: fp32 shards are on split-A with f16 pairs from 32 frames on
    if storage == "fp32":
        split = nf >= 32
        path, name = ("h16", "f16x2") if split else ("fp32", "fp32")
    else:
        split = False
        path, name = {"bf16": ("b16", "bf16-storage"), "f16s": ("s16", "f16-storage"),
                      "sparse": (None, "sparse-fp32")}[storage]
    assert p["nf"] == nf and p["sparse"] == (storage == "sparse") and p["split_a"] == split
    assert (p["fwd"], p["bwd"]) == (path, path)
    assert p["xblk"] == (path not in (None, "fp32"))
    assert (p["forward_split"], p["backproject_split"]) == (name, name)
    cap = {16: 64, 32: 128, 64: 256, 128: 256}[nf]
    assert (p["qcap"], p["rcap"]) == (cap, cap)
    assert p["admit_cap"] == {16: 4, 32: 8, 64: 16, 128: 32}[nf]
    # rule 8 and the rest of the policy
    assert (p["src_age"], p["src_extrap"], p["src_finished"], p["lead"]) == (3, 4.0, False, True)
    assert (p["drift"], p["stage_window"], p["skip_last_bwd"], p["use_graph"], p["fault_nan"]) == (0.0, 0, True, True, -1)
    assert p["chunks"] == [0, 1024] and p["collectives"] == []
    assert p["nwb"] == 11  # 704 rows in blocks of 64
    if storage == "sparse":
        assert (p["nsf"], p["nsb"], p["fplan"], p["bplan"]) == (1, 1, None, None)
        assert p["pw"] == min(nf, 64) and p["needs_w_planes"] == (nf >= 64)
    else:
        assert (p["pw"], p["needs_w_planes"]) == (0, False)


@pytest.mark.parametrize("frames,env,split_a,nf,fwd,bwd", [
    (128, {}, -1, 128, "f16x2", "f16x2"),
    (128, {"SART_MF_BWD16": "0"}, -1, 64, "f16x2", "bf16x3"),
    (128, {}, 0, 64, "fp32", "fp32"),
    (64, {"SART_MF_X3": "0"}, -1, 64, "fp32", "fp32"),
    (64, {"SART_MF_FWD16": "0"}, -1, 64, "bf16x2", "f16x2"),
    (16, {}, 1, 16, "f16x2", "f16x2"),
    (16, {"SART_MF_X3": "1"}, -1, 16, "f16x2", "f16x2"),
    (64, {"SART_MF_X3": "1"}, 0, 64, "fp32", "fp32"),  # EngineConfig::mf_split_a wins over the environment
])
def test_clamp_and_split(k, monkeypatch, frames, env, split_a, nf, fwd, bwd):
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    p = plan(k, "fp32", frames, mf_split_a=split_a)
    assert (p["nf"], p["forward_split"], p["backproject_split"]) == (nf, fwd, bwd)
    assert p["split_a"] == (fwd != "fp32") and p["xblk"] == (fwd != "fp32")
    assert (p["fwd"], p["bwd"]) == tuple({"f16x2": "h16", "bf16x2": "x3", "bf16x3": "x3", "fp32": "fp32"}[s]
                                         for s in (fwd, bwd))


def test_sparse_ignores_split_a(k, monkeypatch):
    monkeypatch.setenv("SART_MF_X3", "1")
    p = plan(k, "sparse", 128, mf_split_a=1)
    assert (p["nf"], p["split_a"], p["xblk"], p["fwd"], p["bwd"]) == (128, False, False, None, None)


@pytest.mark.parametrize("storage,shape,check_interval,chunk", [
    ("fp32", dict(nrows=64, nrows_pad=64, ld=1024), 16, 29),
    ("bf16", dict(nrows=16384, nrows_pad=16384, ld=16384), 16, 6),
    ("fp32", dict(nrows=65536, nrows_pad=65536, ld=65536), 16, 4),
    ("fp32", dict(nrows=65536, nrows_pad=65536, ld=65536), 2, 2),
    ("fp32", dict(nrows=65536, nrows_pad=65536, ld=65536), 0, 1),  # check_interval is at least 1
    ("sparse", dict(nnz=10**6), 16, 28),
])
def test_chunk_length(k, monkeypatch, storage, shape, check_interval, chunk):
    assert plan(k, storage, check_interval=check_interval, **shape)["chunk"] == chunk
    monkeypatch.setenv("SART_MF_CHUNK", "7")
    assert plan(k, storage, check_interval=check_interval, **shape)["chunk"] == 7
    monkeypatch.setenv("SART_MF_CHUNK", "0")
    assert plan(k, storage, check_interval=check_interval, **shape)["chunk"] == 1


def test_queue_capacities(k):
    p = plan(k, "fp32", 128)
    assert (p["nf"], p["qcap"], p["rcap"]) == (128, 256, 256)
    # 256 pinned rows of 8 MiB pass 1 GiB; 128 (= 2 nf) do not
    p = plan(k, "fp32", 64, nrows=1048576, nrows_pad=1048576)
    assert (p["qcap"], p["rcap"]) == (128, 256)
    p = plan(k, "fp32", 64, ld=2097152)
    assert (p["qcap"], p["rcap"]) == (256, 128)
    # never below 2 nf, however large the rows
    p = plan(k, "sparse", 16, nrows=1 << 26, nrows_pad=1 << 26, ld=1 << 27)
    assert (p["qcap"], p["rcap"]) == (32, 32)


def test_voxel_chunks(k, monkeypatch):
    assert plan(k, "fp32", 64, ld=65536)["chunks"] == [0, 65536]
    p = plan(k, "fp32", 64, ld=65536, ranks=2)
    assert p["vox_align"] == p["bplan"]["vox_align"] == 64
    assert p["chunks"] == [0, 16384, 32768, 49152, 65536]
    big = 64 * 65536
    assert p["collectives"] == [big + 64, big, 64, 16384 * 64, 16384 * 64, 16384 * 64, 16384 * 64 + 64]
    # a chunk holds at least 1 MiB of corrections: 16384 voxels at 16 frames
    p = plan(k, "fp32", 16, ld=1024, ranks=2)
    assert p["chunks"] == [0, 1024] and p["collectives"] == [16 * 1024 + 16, 16 * 1024, 16, 16 * 1024 + 16]
    assert plan(k, "fp32", 16, ld=32768, ranks=2)["chunks"] == [0, 16384, 32768]
    monkeypatch.setenv("SART_MF_CHUNKS", "1")
    assert plan(k, "fp32", 64, ld=65536, ranks=2)["chunks"] == [0, 65536]
    # bounds strictly increasing, inner bounds on the alignment (fp32 MFMA at 32 frames: 128-voxel waves)
    monkeypatch.setenv("SART_MF_CHUNKS", "7")
    # (66752 = 1043 x 64 is no multiple of 128, 66816 = 522 x 128 is; 16 frames: 4 chunks of >= 16384 voxels fit)
    for storage, frames, ld, align, n in (("fp32", 32, 66752, 64, 7), ("fp32", 32, 66816, 128, 7),
                                          ("bf16", 64, 66816, 128, 7), ("sparse", 32, 66816, 128, 7),
                                          ("sparse", 16, 66816, 64, 4), ("sparse", 64, 66752, 64, 7)):
        p = plan(k, storage, frames, ld=ld, ranks=3, mf_split_a=0)
        c = p["chunks"]
        assert p["vox_align"] == align and c[0] == 0 and c[-1] == ld and len(c) == n + 1, (storage, frames, ld)
        assert all(a < b for a, b in zip(c, c[1:])) and all(v % align == 0 for v in c[1:-1])
        if storage != "sparse":
            assert p["bplan"]["vox_align"] == align


# (variable, value, plan arguments, field, value with the variable set, default)
KNOB_CASES = [
    ("SART_MF_X3", "0", {}, "split_a", False, True),
    ("SART_MF_BWD16", "0", {}, "bwd", "x3", "h16"),
    ("SART_MF_FWD16", "0", {}, "fwd", "x3", "h16"),
    ("SART_MF_XBLK", "0", {}, "xblk", False, True),
    ("SART_MF_LAST_BWD", "1", {}, "skip_last_bwd", False, True),
    ("SART_MF_CHUNK", "7", {}, "chunk", 7, 29),  # 704 x 1024 fp32: t = 5.3153e-5, 28.22 -> 29
    ("SART_MF_GRAPH", "0", {}, "use_graph", False, True),
    ("SART_MF_ADMIT_CAP", "3", {}, "admit_cap", 3, 16),
    ("SART_MF_ADMIT_CAP", "-5", {}, "admit_cap", 0, 16),
    ("SART_MF_SRC_AGE", "5", {}, "src_age", 5, 3),
    ("SART_MF_SRC_AGE", "-1", {}, "src_age", 0, 3),
    ("SART_MF_SRC_FINISHED", "1", {}, "src_finished", True, False),
    ("SART_MF_LEAD", "0", {}, "lead", False, True),
    ("SART_MF_SRC_EXTRAP", "2.5", {}, "src_extrap", 2.5, 4.0),
    ("SART_MF_DRIFT", "1.5", {}, "drift", 1.5, 0.0),
    ("SART_MF_STAGE_WINDOW", "2", {}, "stage_window", 2, 0),
    ("SART_MF_STAGE_WINDOW", "-2", {}, "stage_window", 0, 0),
    ("SART_MF_CHUNKS", "2", dict(ld=65536, ranks=2), "chunks", [0, 32768, 65536], [0, 16384, 32768, 49152, 65536]),
    ("SART_FAULT_NAN", "3", {}, "fault_nan", 3, -1),
    ("SART_MF_SPARSE_PW", "16", dict(storage="sparse"), "pw", 16, 64),
]


def test_knob_cases_cover_every_variable():
    assert {c[0] for c in KNOB_CASES} == set(ENGINE_KNOBS) and len(ENGINE_KNOBS) == 17


@pytest.mark.parametrize("name,value,args,field,expected,default", KNOB_CASES)
def test_knob_parsing(k, monkeypatch, name, value, args, field, expected, default):
    assert plan(k, **args)[field] == default
    monkeypatch.setenv(name, value)
    assert plan(k, **args)[field] == expected
    monkeypatch.setenv(name, "")
    assert plan(k, **args)[field] == default


def test_sparse_plane_width(k, monkeypatch):
    p = plan(k, "sparse", 128)
    assert (p["pw"], p["needs_w_planes"]) == (64, True)
    p = plan(k, "sparse", 32)
    assert (p["pw"], p["needs_w_planes"]) == (32, False)
    monkeypatch.setenv("SART_MF_SPARSE_PW", "32")
    p = plan(k, "sparse", 32)
    assert (p["pw"], p["needs_w_planes"]) == (32, False)
    p = plan(k, "sparse", 16)
    assert (p["pw"], p["needs_w_planes"]) == (16, False)
    monkeypatch.setenv("SART_MF_SPARSE_PW", "16")
    p = plan(k, "sparse", 64)
    assert (p["pw"], p["needs_w_planes"]) == (16, True)
    monkeypatch.setenv("SART_MF_SPARSE_PW", "48")
    with pytest.raises(RuntimeError, match="SART_MF_SPARSE_PW must be 16, 32 or 64"):
        plan(k, "sparse", 64)
    assert plan(k, "fp32", 64)["pw"] == 0  # a dense shard has no planes: the variable is not looked at


@pytest.mark.parametrize("ld,nrows", [(1024, 700), (2048, 1000), (65536, 16384)])
@pytest.mark.parametrize("storage,frames,env", [
    ("fp32", 16, {}), ("fp32", 64, {}), ("fp32", 128, {}), ("fp32", 64, {"SART_MF_FWD16": "0", "SART_MF_BWD16": "0"}),
    ("fp32", 64, {"SART_MF_X3_VT": "2", "SART_MF_BP_BLOCKS": "64"}), ("bf16", 128, {}), ("bf16", 32, {}),
    ("f16s", 128, {}),
])
def test_launch_plans(k, monkeypatch, storage, frames, env, ld, nrows):
    """fplan / bplan are mf_plan_forward / mf_plan_backproject of the plan's paths and sizes under the same launch
    knobs, and the slice counts the engine allocates for are theirs."""
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    pad = (nrows + 63) // 64 * 64
    p = plan(k, storage, frames, nrows=nrows, nrows_pad=pad, ld=ld)
    assert p["fplan"] == k.mf_plan_forward(p["fwd"], p["nf"], ld, pad)
    assert p["bplan"] == k.mf_plan_backproject(p["bwd"], p["nf"], ld, nrows)
    assert (p["nsf"], p["nsb"]) == (p["fplan"]["nsplit"], p["bplan"]["nsplit"])
    assert p["vox_align"] == p["bplan"]["vox_align"]


def test_untabled_launch_knobs_are_refused(k, monkeypatch):
    monkeypatch.setenv("SART_MF_DEPTH", "1")  # no f16-storage kernel with a ring of 1
    with pytest.raises(RuntimeError, match="s16 path: no kernel"):
        plan(k, "f16s", 64)
