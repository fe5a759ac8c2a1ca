"""The launch planner of the multi-frame MFMA projections (csrc/engine/mf_plan.cpp) on the CPU: default plans against
the rules written out here, the knob settings the suite and the A/B notes use, the refusal of untabled combinations,
ignored malformed values, and the consistency of what the engine allocates with what a launch covers."""
import itertools

import pytest

from mpi_cuda_sartsolver_amd.ops import hip

KNOBS = ("SART_MF_DEPTH", "SART_MF_ROWS", "SART_MF_VOX", "SART_MF_NT", "SART_MF_B16_FWD", "SART_MF_B16_VT",
         "SART_MF_X3_FWD", "SART_MF_X3_DEPTH", "SART_MF_X3_VT", "SART_MF_XEARLY", "SART_MF_WEARLY", "SART_MF_H16",
         "SART_MF_H16_FDEPTH", "SART_MF_FWD_BLOCKS", "SART_MF_BP_BLOCKS")
LDS = (1024, 1088, 65536, 131072, 262144)
PADS_ODD32 = (32, 96, 1056)            # 32 k, k odd: the fallback tiles
PADS_64 = (64, 1024, 16384, 65536)     # 64 k
ROWS = (64, 700, 1000, 16384, 65536)
PATHS = ("fp32", "b16", "x3", "h16")
FWD_NF = {"fp32": (16, 32, 64), "b16": (16, 32, 64, 128), "x3": (16, 32, 64, 128), "h16": (16, 32, 64, 128)}
BWD_NF = {"fp32": (16, 32, 64), "b16": (16, 32, 64, 128), "x3": (16, 32, 64), "h16": (16, 32, 64, 128)}

# Split counts of the parent commit's mf_forward_num_splits / mf_backproject*_num_splits (pure host arithmetic,
# recorded from its build with no knob set).
FWD_SPLITS = {  # (ld, nrows_pad): (target 1024, target 512 of bf16 storage)
    (1024, 32): (1, 1), (1024, 96): (1, 1), (1024, 1056): (1, 1), (1024, 64): (1, 1), (1024, 1024): (1, 1),
    (1024, 16384): (1, 1), (1024, 65536): (1, 1),
    (1088, 32): (1, 1), (1088, 96): (1, 1), (1088, 1056): (1, 1), (1088, 64): (1, 1), (1088, 1024): (1, 1),
    (1088, 16384): (1, 1), (1088, 65536): (1, 1),
    (65536, 32): (64, 64), (65536, 96): (64, 64), (65536, 1056): (64, 57), (65536, 64): (64, 64),
    (65536, 1024): (64, 64), (65536, 16384): (16, 8), (65536, 65536): (4, 2),
    (131072, 32): (128, 128), (131072, 96): (128, 128), (131072, 1056): (114, 57), (131072, 64): (128, 128),
    (131072, 1024): (128, 128), (131072, 16384): (16, 8), (131072, 65536): (4, 2),
    (262144, 32): (256, 256), (262144, 96): (256, 256), (262144, 1056): (114, 57), (262144, 64): (256, 256),
    (262144, 1024): (256, 128), (262144, 16384): (16, 8), (262144, 65536): (4, 2),
}
BWD_SPLITS = {  # (ld, nrows): (fp32, bf16 storage, split-A)
    (1024, 64): (1, 1, 1), (1024, 700): (11, 11, 11), (1024, 1000): (16, 16, 16), (1024, 16384): (256, 256, 256),
    (1024, 65536): (1024, 1024, 256),
    (1088, 64): (1, 1, 1), (1088, 700): (11, 11, 11), (1088, 1000): (16, 16, 16), (1088, 16384): (256, 256, 205),
    (1088, 65536): (410, 410, 205),
    (65536, 64): (1, 1, 1), (65536, 700): (11, 11, 4), (65536, 1000): (16, 16, 4), (65536, 16384): (16, 16, 4),
    (65536, 65536): (16, 16, 4),
    (131072, 64): (1, 1, 1), (131072, 700): (8, 8, 2), (131072, 1000): (8, 8, 2), (131072, 16384): (8, 8, 2),
    (131072, 65536): (8, 8, 2),
    (262144, 64): (1, 1, 1), (262144, 700): (4, 4, 1), (262144, 1000): (4, 4, 1), (262144, 16384): (4, 4, 1),
    (262144, 65536): (4, 4, 1),
}


@pytest.fixture
def k(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return hip()


def _key(plan):
    return {f: plan[f] for f in ("path", "forward", "ng", "depth", "tile", "kb", "lds", "as", "early", "nt", "mw")}


def _fwd(path, nf, depth, rt, kb=0, lds=False, staged=False, early=False, nt=False):
    return dict(path=path, forward=True, ng=nf // 16, depth=depth, tile=rt, kb=kb, lds=lds, early=early, nt=nt, mw=0,
                **{"as": staged})


def _bwd(path, nf, depth, vt, lds=False, early=False, mw=0):
    return dict(path=path, forward=False, ng=nf // 16, depth=depth, tile=vt, kb=0, lds=lds, early=early, nt=False,
                mw=mw, **{"as": False})


def _default_forward(path, nf, ld, pad):
    if path == "fp32":  # RT 4 (RT 2 where the padded rows are no multiple of 64), depth 2 at 64 frames and 3 otherwise
        return _fwd(path, nf, 2 if nf == 64 else 3, 4 if pad % 64 == 0 else 2)
    if path == "b16":  # 16: (2,2,lds); 32: (2,2,lds,as); 64: (4,2,lds); 128: (2,2,lds,as); depth 3; X with A
        rt, kb, staged = {16: (2, 2, False), 32: (2, 2, True), 64: (4, 2, False), 128: (2, 2, True)}[nf]
        if pad % (16 * rt) != 0:  # a wave's rows inside the padding: (2, 1), not staged
            rt, kb, staged = 2, 1, False
        if nf == 128:
            rt, kb, staged = 2, 2, True
        return _fwd(path, nf, 3, rt, kb, True, staged, False)
    # split-A: 32 / 64 frames RT 2, KB 1 below 131072 columns and 2 from there, A staged; 16 frames (2, 2), not
    # staged; 128 frames (2, 1), staged; X in LDS and early, depth 2
    kb, staged = {16: (2, False), 32: (2 if ld >= 131072 else 1, True), 64: (2 if ld >= 131072 else 1, True),
                  128: (1, True)}[nf]
    return _fwd(path, nf, 2, 2, kb, True, staged, True)


def _default_backproject(path, nf, ld):
    if path == "fp32":  # VT 2 from 32 frames on where ld % 128 == 0; depth 1 at 32 frames, else 2
        return _bwd(path, nf, 1 if nf == 32 else 2, 2 if nf >= 32 and ld % 128 == 0 else 1)
    if path == "b16":  # VT 2 iff ld % 128 == 0 and nf != 128; W in LDS, W early, depth 3
        return _bwd(path, nf, 3, 2 if ld % 128 == 0 and nf != 128 else 1, True, True)
    if path == "x3":  # VT 1, depth 2, W not early
        return _bwd(path, nf, 2, 1, True, False)
    return _bwd(path, nf, 2, 1, True, False, 1 if nf == 128 else 2)  # h16: depth 2, MW 2; 128 frames MW 1


def test_default_plans(k):
    for path, ld in itertools.product(PATHS, LDS):
        for nf in FWD_NF[path]:
            for pad in (PADS_64 if path == "h16" else PADS_ODD32 + PADS_64):
                p = k.mf_plan_forward(path, nf, ld, pad)
                assert _key(p) == _default_forward(path, nf, ld, pad), (path, nf, ld, pad)
                assert p["nsplit"] == FWD_SPLITS[(ld, pad)][1 if path == "b16" else 0], (path, nf, ld, pad)
                assert p["grid"] == (-(-pad // (64 * p["tile"])), p["nsplit"])
                unit = 16 if path == "fp32" else 64
                assert p["cps"] % unit == 0 and p["cps"] * p["nsplit"] >= ld > p["cps"] * (p["nsplit"] - 1) - unit
        for nf in BWD_NF[path]:
            for rows in ROWS:
                p = k.mf_plan_backproject(path, nf, ld, rows)
                assert _key(p) == _default_backproject(path, nf, ld), (path, nf, ld, rows)
                assert p["nsplit"] == BWD_SPLITS[(ld, rows)][PATHS.index(path) if path != "h16" else 2]
        assert k.mf_forward_num_splits(ld, 1024) == FWD_SPLITS[(ld, 1024)][0]
        assert k.mf_forward_num_splits(ld, 1024, 512) == FWD_SPLITS[(ld, 1024)][1]
        assert (k.mf_backproject_num_splits(ld, 1000), k.mf_backproject_b16_num_splits(ld, 1000),
                k.mf_backproject_b16_num_splits(ld, 1000, True)) == BWD_SPLITS[(ld, 1000)]
        assert k.mf_backproject_b16_vox_align(ld) == (128 if ld % 128 == 0 else 64)
        assert k.mf_backproject_b16_vox_align(ld, True) == 64


def _plan_everything(k, paths):
    """Every plan of `paths` over the shapes above; returns the keys."""
    keys = []
    for path, ld in itertools.product(paths, (1024, 1088, 131072)):
        for nf in FWD_NF[path]:
            for pad in ((64, 1024) if path == "h16" else (32, 64, 96, 1024)):
                keys.append(_key(k.mf_plan_forward(path, nf, ld, pad)))
        for nf in BWD_NF[path]:
            keys.append(_key(k.mf_plan_backproject(path, nf, ld, 1000)))
    return keys


def _in_table(k, key):
    nf = 16 * key["ng"]
    return any(_key(v) == key for v in k.mf_variants(key["path"], nf, key["forward"]))


# the parametrisations of tests/test_gpu_multiframe_bf16.py and the setters of tests/test_gpu_kernels.py
SUITE_SETTINGS = (
    [(("b16",), {"SART_MF_B16_FWD": f, "SART_MF_B16_VT": b})
     for f, b in (("4,1", "1,reg"), ("8,1", "2,reg"), ("4,2,lds", "1,lds"), ("8,1,lds", "2,lds"), ("2,2,lds", "2,lds"),
                  ("4,2,lds,as", "2,lds"), ("2,2,lds,as", "1,lds"))] +
    [(("x3", "h16"), {"SART_MF_X3_FWD": f, "SART_MF_X3_VT": v, "SART_MF_X3_DEPTH": d})
     for f, v, d in (("2,1", "1", "3"), ("2,2", "2", "2"), ("4,2", "2", "3"), ("4,1,as", "1", "2"), ("2,2,as", "1", "3"),
                     ("2,1,as", "2", "2"))] +
    [(("x3", "h16"), {"SART_MF_X3_FWD": f}) for f in ("2,2", "4,1,as", "2,2,as")] +
    [(("b16",), {"SART_MF_B16_FWD": f}) for f in ("4,1", "8,1,lds", "2,2,lds,as")])
# each A/B knob alone against the defaults
SINGLE_KNOBS = (
    [(("fp32", "b16"), {"SART_MF_DEPTH": d}) for d in "123"] +
    [(("fp32",), {"SART_MF_ROWS": r}) for r in "24"] + [(("fp32",), {"SART_MF_VOX": v}) for v in "12"] +
    [(("fp32",), {"SART_MF_NT": "1"})] +
    [(("b16",), {"SART_MF_B16_VT": v}) for v in ("1", "2", "1,reg", "2,reg", "1,lds", "2,lds")] +
    [(("x3", "h16"), {"SART_MF_X3_DEPTH": d}) for d in "23"] + [(("x3", "h16"), {"SART_MF_X3_VT": v}) for v in "12"] +
    [(("b16", "x3"), {"SART_MF_XEARLY": v}) for v in "01"] + [(("b16", "x3"), {"SART_MF_WEARLY": v}) for v in "01"] +
    [(("h16",), {"SART_MF_H16": v}) for v in ("ew", "w1", "ew,w1")] + [(("h16",), {"SART_MF_H16_FDEPTH": "3"})])


@pytest.mark.parametrize("paths,env", SUITE_SETTINGS + SINGLE_KNOBS, ids=lambda v: str(v).replace(" ", ""))
def test_named_knob_settings_are_tabled(k, monkeypatch, paths, env):
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    for key in _plan_everything(k, paths):  # planning throws for a key outside the table
        assert _in_table(k, key), key


def test_knob_values_reach_the_plan(k, monkeypatch):
    monkeypatch.setenv("SART_MF_X3_FWD", "4,2")
    monkeypatch.setenv("SART_MF_X3_DEPTH", "3")
    assert _key(k.mf_plan_forward("x3", 64, 2048, 1024)) == _fwd("x3", 64, 3, 4, 2, True, False, True)
    assert _key(k.mf_plan_forward("x3", 64, 2048, 96)) == _fwd("x3", 64, 3, 2, 1, True, False, True)  # 96 % 64
    assert _key(k.mf_plan_forward("h16", 64, 2048, 1024)) == _fwd("h16", 64, 2, 2, 2, True, False, True)
    monkeypatch.delenv("SART_MF_X3_DEPTH")
    monkeypatch.setenv("SART_MF_H16", "ew,w1")
    assert _key(k.mf_plan_backproject("h16", 32, 2048, 1000)) == _bwd("h16", 32, 2, 1, True, True, 1)
    monkeypatch.setenv("SART_MF_B16_VT", "1,reg")
    assert _key(k.mf_plan_backproject("b16", 32, 2048, 1000)) == _bwd("b16", 32, 3, 1, False, False)
    monkeypatch.setenv("SART_MF_BP_BLOCKS", "64")
    monkeypatch.setenv("SART_MF_FWD_BLOCKS", "8")
    assert k.mf_plan_backproject("b16", 32, 65536, 16384)["nsplit"] == 1 == k.mf_backproject_b16_num_splits(65536, 16384)
    assert k.mf_plan_backproject("fp32", 32, 1024, 16384)["nsplit"] == 32 == k.mf_backproject_num_splits(1024, 16384)
    assert k.mf_plan_forward("x3", 32, 65536, 1024)["nsplit"] == 2 == k.mf_forward_num_splits(65536, 1024)
    # the setters win over the environment; 0 hands it back
    monkeypatch.setenv("SART_MF_ROWS", "2")
    k.mf_set_rows(4)
    k.mf_set_depth(1)
    try:
        assert _key(k.mf_plan_forward("fp32", 16, 1024, 1024)) == _fwd("fp32", 16, 1, 4)
    finally:
        k.mf_set_rows(0)
        k.mf_set_depth(0)
    assert _key(k.mf_plan_forward("fp32", 16, 1024, 1024)) == _fwd("fp32", 16, 3, 2)


@pytest.mark.parametrize("path,env", [
    ("b16", {"SART_MF_B16_FWD": "8,1", "SART_MF_DEPTH": "1", "SART_MF_XEARLY": "1"}),
    ("b16", {"SART_MF_B16_FWD": "8,1,lds", "SART_MF_DEPTH": "1", "SART_MF_XEARLY": "1"}),
    ("x3", {"SART_MF_X3_FWD": "4,1", "SART_MF_X3_DEPTH": "3", "SART_MF_XEARLY": "0"}),
    ("fp32", {"SART_MF_NT": "1", "SART_MF_DEPTH": "1"}),
])
def test_untabled_combination_raises(k, monkeypatch, path, env):
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    with pytest.raises(RuntimeError) as err:
        k.mf_plan_forward(path, 16, 2048, 1024)
    for name, val in env.items():
        assert "%s=%s" % (name, val) in str(err.value), str(err.value)
    assert path + " path" in str(err.value)


@pytest.mark.parametrize("env", [{"SART_MF_X3_FWD": "3,1"}, {"SART_MF_DEPTH": "9"}, {"SART_MF_B16_FWD": "16,2,lds"},
                                 {"SART_MF_B16_FWD": "4,3"}, {"SART_MF_X3_FWD": "8,1"}, {"SART_MF_X3_DEPTH": "1"},
                                 {"SART_MF_B16_VT": "3"}, {"SART_MF_X3_VT": "0"}, {"SART_MF_ROWS": "3"},
                                 {"SART_MF_VOX": "4"}, {"SART_MF_H16_FDEPTH": "4"}, {"SART_MF_DEPTH": ""}])
def test_malformed_values_are_ignored(k, monkeypatch, env):
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    for path, ld in itertools.product(PATHS, (1088, 131072)):
        for nf in FWD_NF[path]:
            assert _key(k.mf_plan_forward(path, nf, ld, 1024)) == _default_forward(path, nf, ld, 1024)
        for nf in BWD_NF[path]:
            assert _key(k.mf_plan_backproject(path, nf, ld, 1000)) == _default_backproject(path, nf, ld)


@pytest.mark.parametrize("env", [{}, {"SART_MF_B16_VT": "1", "SART_MF_X3_VT": "2"}, {"SART_MF_VOX": "1"},
                                 {"SART_MF_BP_BLOCKS": "64", "SART_MF_FWD_BLOCKS": "100000"}])
def test_allocation_matches_launch(k, monkeypatch, env):
    """The engine sizes its partial slices from plan["nsplit"] and aligns its voxel chunks to plan["vox_align"]; the
    launch covers grid = (workgroups, nsplit) with 4 waves of 64 * tile voxels (16 * tile rows) per workgroup."""
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    for path, ld in itertools.product(PATHS, LDS):
        for nf in BWD_NF[path]:
            for rows in ROWS:
                p = k.mf_plan_backproject(path, nf, ld, rows)
                assert p["vox_align"] % (64 * p["tile"]) == 0 and ld % p["vox_align"] == 0
                assert p["grid"] == (-(-(ld // (64 * p["tile"])) // 4), p["nsplit"])
                unit = 16 if path == "fp32" else 32
                assert p["rps"] % unit == 0 and p["rps"] * p["nsplit"] >= rows
        for nf in FWD_NF[path]:
            for pad in PADS_64:
                p = k.mf_plan_forward(path, nf, ld, pad)
                assert p["grid"][1] == p["nsplit"] and p["grid"][0] * 64 * p["tile"] >= pad
                assert pad % (16 * p["tile"]) == 0  # a wave's rows lie inside the padding
                assert p["cps"] * p["nsplit"] >= ld
