"""The launch planner of the single-frame fused sweep (csrc/engine/fused_plan.cpp) on the CPU: which kernel runs for a
geometry, a storage and the knobs, against the rules written out here; the split flag the engine sizes its partial
rows from; the refusals and shape checks of a launch; and the size of the kernel tables
(csrc/engine/fused_variants.hpp)."""
import pytest

from mpi_cuda_sartsolver_amd.models import rtm
from mpi_cuda_sartsolver_amd.ops import hip

CUS = 256  # MI355X: 8 XCDs x 32 CUs
KNOBS = ("SART_FUSED_CW_SCHED", "SART_BF16_T2_SCHED", "SART_FUSED_GPAD", "SART_FUSED_CW_MAP")
GEOMETRY_ENV = ("SART_FUSED_T", "SART_BF16_WIDE", "SART_FUSED_XL", "SART_BF16_XL", "SART_BF16_KW", "SART_FUSED_SEG")
STORAGES = ("f32", "bf16", "f16")
WIDTHS = list(range(20480, 262145, 997)) + list(range(262144, 1048577, 8191))  # test_geometry.py's width sweep
V6_SCHEDULES = [(4, 0), (4, 1), (4, 2), (4, 3), (4, 4), (2, 1), (2, 2), (2, 4), (1, 0), (1, 4), (1, 5)]  # test_gpu_solver.py


@pytest.fixture
def k(monkeypatch):
    for name in KNOBS + GEOMETRY_ENV:
        monkeypatch.delenv(name, raising=False)
    lib = hip()
    prev = lib.fused_get_schedule()
    lib.fused_set_schedule(4)
    lib.fused_set_debug(0)
    yield lib
    lib.fused_set_schedule(prev)
    lib.fused_set_debug(0)


def _geometry(k, nvox, storage, T=0, wide=True):
    """The geometry Engine plans for a shard of nvox voxels (engine.cpp): fp32 shards take fused_geometry with the
    narrow slabs and chip-wide groups, 16-bit shards the wide tiles where the width allows (unless SART_BF16_WIDE=0
    or T is forced to 1 or 2), else the narrow ones in XCD-local groups; variant 6 only."""
    ld = rtm.choose_ld(nvox, storage="fp32" if storage == "f32" else "bf16")
    if storage == "f32":
        g = k.fused_geometry(ld, CUS, 6, T)
    else:
        g = k.fused_geometry(ld, CUS, 6, T, False, False)
        if wide and T in (0, 4):
            gw = k.fused_geometry_bf16_wide(ld, CUS)
            if gw.valid():
                g = gw
    return ld, (g if g.valid() and g.variant == 6 else None)


def _made(k, **fields):
    """A geometry fused_geometry never returns (K = T: variant 6 carries the rows per tile in K)."""
    g = k.FusedGeometry()
    g.variant, g.cpl, g.kw, g.xl = 6, 4, 8, True
    for name, v in fields.items():
        setattr(g, name, v)
    g.K, g.grid = g.T, g.I * g.J
    return g


def _expected(g, storage, sched=4, debug=0, cw_sched5=False, t2_sched6=False):
    """(sched, diag) of the kernel that runs. fp32: chip-wide groups run 5 at T = 1 (7- / 6-KiB slabs 8 unless
    SART_FUSED_CW_SCHED=5) and 4 at T >= 2; XCD-local slabs other than 8 KiB run the defaults, 5 at T = 1 and 4 at
    T >= 2; only XCD-local 8-KiB slabs follow fused_set_schedule (T >= 2: 5 means 4; T = 1: 4 and 5 mean 5, else 0) and
    the instrumented build (schedules 2 and 4, else 0). 16-bit: wide tiles 4 at T = 4, 7 at T = 2 (6 with
    SART_BF16_T2_SCHED=6); narrow tiles 4 at T >= 2, 0 at T = 1 (5 under fused_set_schedule(5)); never instrumented."""
    if storage == "f32":
        if not g.xl:
            return (4 if g.T >= 2 else (8 if g.kw in (6, 7) and not cw_sched5 else 5)), False
        if g.kw != 8:
            return (4 if g.T >= 2 else 5), False
        run = (4 if sched == 5 else sched) if g.T >= 2 else (5 if sched >= 4 else 0)
        diag = bool(debug & 2)
        return (run if not diag or run in (2, 4) else 0), diag
    if g.cpl == 8:
        return (4 if g.T == 4 else (6 if t2_sched6 else 7)), False
    return (4 if g.T >= 2 else (5 if sched == 5 else 0)), False


def _check(k, g, storage, **knobs):
    p = k.fused_plan(g, storage)
    sched, diag = _expected(g, storage, **knobs)
    key = dict(storage=storage, variant=6, xl=g.xl, diag=diag, T=g.T, sched=sched, cpl=g.cpl if storage != "f32" else 4,
               kw=g.kw)
    assert {f: p[f] for f in key} == key, (p, key)
    assert p["split"] == (4 <= sched <= 8) and p["threads"] == (384 if p["split"] else 320)
    assert 0 < p["lds_bytes"] <= 160 * 1024
    return p


def test_default_keys_are_built_at_every_width(k, monkeypatch):
    """No reachable width plans a kernel that does not exist: the width sweep of test_geometry.py in all three
    storages, at the planner's T and at T forced to 1, 2 and 4, with wide and (SART_BF16_WIDE=0) narrow 16-bit tiles."""
    seen = {s: set() for s in STORAGES}
    for nvox in WIDTHS:
        for storage in STORAGES:
            for T, wide in [(0, True), (1, True), (2, True), (4, True), (0, False)]:
                if storage == "f32" and not wide:
                    continue
                _, g = _geometry(k, nvox, storage, T, wide)
                if g is None:  # (a forced T or the narrow tiles cannot split every width: the two-pass kernels run)
                    assert T != 0 or not wide, (nvox, storage)
                    continue
                p = _check(k, g, storage)
                assert p["built"], (nvox, storage, T, p)
                seen[storage].add((g.xl, g.T, p["sched"], g.cpl, g.kw))
    # fp32 T >= 2 runs schedule 4, T = 1 schedule 5, chip-wide 7- / 6-KiB slabs schedule 8
    assert {(T, s) for _, T, s, _, _ in seen["f32"]} == {(1, 5), (1, 8), (2, 4), (4, 4)}
    assert all(s != 8 or (not xl and kw in (6, 7)) for xl, _, s, _, kw in seen["f32"])
    # bf16 / f16: wide T = 4 schedule 4, wide T = 2 schedule 7, narrow T = 1 schedule 0, narrow T >= 2 schedule 4
    for storage in ("bf16", "f16"):
        assert {(T, s, cpl) for _, T, s, cpl, _ in seen[storage]} == {(4, 4, 8), (2, 7, 8), (1, 0, 4), (2, 4, 4), (4, 4, 4)}
    assert seen["bf16"] == seen["f16"]


@pytest.mark.parametrize("T,sched", V6_SCHEDULES)
def test_set_schedule_pairs_of_the_gpu_suite(k, T, sched):
    """Every (T, sched) of test_fused_v6_schedules at its 16384-voxel shard: 8-KiB slabs in XCD-local groups, so the
    schedule set is the schedule run, except 5 at T >= 2 (runs 4) and 1-4 at T = 1 (4 runs 5, the others 0)."""
    g = k.fused_geometry(rtm.choose_ld(16384), CUS, 6, T)
    assert g.variant == 6 and g.T == T and g.xl and g.kw == 8
    k.fused_set_schedule(sched)
    p = _check(k, g, "f32", sched=sched)
    assert p["built"] and p["sched"] == {(1, 4): 5}.get((T, sched), sched)


def test_schedules_without_a_kernel_of_their_own(k):
    for T in (2, 4):
        k.fused_set_schedule(5)
        assert _check(k, k.fused_geometry(65536, CUS, 6, T), "f32", sched=5)["sched"] == 4
    g1 = k.fused_geometry(65536, CUS, 6, 1)
    for sched in (0, 1, 2, 3):
        k.fused_set_schedule(sched)
        assert _check(k, g1, "f32", sched=sched)["sched"] == 0
    # fused_set_schedule reaches neither other slab widths nor chip-wide groups nor 16-bit tiles (but narrow T = 1 at 5)
    for sched in range(6):
        k.fused_set_schedule(sched)
        for ld, storage in [(100352, "f32"), (150528, "f32"), (524288, "f32")]:
            g = k.fused_geometry(ld, CUS, 6, 0)
            assert g.kw != 8 or not g.xl
            assert _check(k, g, storage, sched=sched)["built"]
        for storage in ("bf16", "f16"):
            assert _check(k, k.fused_geometry_bf16_wide(65536, CUS), storage, sched=sched)["built"]
            p = _check(k, k.fused_geometry(65536, CUS, 6, 1, False, False), storage, sched=sched)
            assert p["built"] == (sched != 5 or storage == "bf16")


def test_environment_schedules(k, monkeypatch):
    cw7 = k.fused_geometry(150528, CUS, 6, 0)   # chip-wide 7-KiB slabs at T = 1
    cw8 = k.fused_geometry(524288, CUS, 6, 0)   # chip-wide 8-KiB slabs
    assert (cw7.xl, cw7.T, cw7.kw, cw8.xl, cw8.T, cw8.kw) == (False, 1, 7, False, 1, 8)
    assert _check(k, cw7, "f32")["sched"] == 8 and _check(k, cw8, "f32")["sched"] == 5
    monkeypatch.setenv("SART_FUSED_CW_SCHED", "5")
    p = _check(k, cw7, "f32", cw_sched5=True)
    assert p["sched"] == 5 and p["built"] and _check(k, cw8, "f32", cw_sched5=True)["sched"] == 5
    t2 = k.fused_geometry_bf16_wide(524288, CUS)
    assert (t2.cpl, t2.T) == (8, 2)
    monkeypatch.setenv("SART_BF16_T2_SCHED", "6")
    p = _check(k, t2, "bf16", t2_sched6=True)
    assert p["sched"] == 6 and p["built"] and p["split"]
    assert _check(k, k.fused_geometry_bf16_wide(65536, CUS), "bf16", t2_sched6=True)["sched"] == 4  # T = 4: untouched
    monkeypatch.setenv("SART_BF16_T2_SCHED", "7")
    assert _check(k, t2, "bf16")["sched"] == 7


@pytest.mark.parametrize("sched", range(6))
def test_instrumented_build(k, sched):
    """fused_set_debug(2) selects the instrumented kernels for fp32 XCD-local 8-KiB slabs only: schedules 2 and 4
    (T >= 2), else schedule 0. Everywhere else the flag reaches the kernel's dbg argument and selects nothing."""
    k.fused_set_schedule(sched)
    k.fused_set_debug(2)
    for T in (1, 2, 4):
        p = _check(k, k.fused_geometry(65536, CUS, 6, T), "f32", sched=sched, debug=2)
        assert p["diag"] and p["built"] and p["dbg"] & 2
        assert p["sched"] == (sched if T >= 2 and sched in (2, 4) else (4 if T >= 2 and sched == 5 else 0))
    ignored = [(k.fused_geometry(100352, CUS, 6, 0), "f32"), (k.fused_geometry(150528, CUS, 6, 0), "f32"),
               (k.fused_geometry_bf16_wide(65536, CUS), "bf16"), (k.fused_geometry_bf16_wide(65536, CUS), "f16"),
               (k.fused_geometry(65536, CUS, 6, 4, False, False), "bf16")]
    for g, storage in ignored:
        p = _check(k, g, storage, sched=sched, debug=2)
        assert not p["diag"] and p["built"] and p["dbg"] & 2


def test_debug_bits_of_the_group_map_and_granule_padding(k, monkeypatch):
    xl = k.fused_geometry(65536, CUS, 6, 4)
    even, odd = k.fused_geometry(524288, CUS, 6, 0), _made(k, T=1, J=51, I=5, xl=False)
    assert even.I % 2 == 0 and not even.xl
    assert [k.fused_plan(g, "f32")["dbg"] for g in (xl, even, odd)] == [0, 0, 8]  # balanced map for even I only
    monkeypatch.setenv("SART_FUSED_CW_MAP", "0")
    assert [k.fused_plan(g, "f32")["dbg"] for g in (xl, even, odd)] == [0, 8, 8]
    monkeypatch.setenv("SART_FUSED_CW_MAP", "1")
    assert [k.fused_plan(g, "f32")["dbg"] for g in (xl, even, odd)] == [0, 0, 0]
    monkeypatch.setenv("SART_FUSED_GPAD", "0")
    assert [k.fused_plan(g, "f32")["dbg"] for g in (xl, even)] == [0, 16]
    monkeypatch.setenv("SART_FUSED_GPAD", "2")
    assert [k.fused_plan(g, "f32")["dbg"] for g in (xl, even)] == [32, 0]


def test_split_is_what_the_engine_sizes_its_partial_rows_from(k, monkeypatch):
    """FusedPlan.split is the single definition of a split schedule (4 ... 8): the chain plan computed from it gives the
    block counts test_geometry.py::test_segment_plan pins, and it follows the kernel that runs, not the schedule set."""
    g4 = k.fused_geometry(65536, CUS, 6, 4)
    monkeypatch.setenv("SART_BF16_XL", "1")
    gw = k.fused_geometry_bf16_wide(262144, CUS)  # XCD-local T = 2, I = 8: 32768 tiles per group at 512k rows
    assert (gw.T, gw.xl, gw.I) == (2, True, 8)
    p4, pw = k.fused_plan(g4, "f32"), k.fused_plan(gw, "bf16")
    assert pw["split"] and p4["split"]  # bf16 T = 2 and fp32 T = 4 are split by default
    assert k.fused_chain_plan(g4, 65536, p4["split"]) == (0, g4.I)
    assert k.fused_chain_plan(gw, 524288, pw["split"]) == (700, 8 * 2 * 47)
    assert k.fused_chain_plan(gw, 524288, k.fused_plan(gw, "f16")["split"]) == (700, 8 * 2 * 47)
    k.fused_set_schedule(2)
    p2 = k.fused_plan(g4, "f32")
    assert p2["sched"] == 2 and not p2["split"] and k.fused_chain_plan(g4, 524288, p2["split"]) == (0, g4.I)
    # ... while chip-wide groups and other slab widths keep schedule 4, whatever is set: split
    cw = _made(k, T=4, J=64, I=4, xl=False)
    kw7 = _made(k, T=2, J=28, I=8, kw=7)
    for g in (cw, kw7):
        p = k.fused_plan(g, "f32")
        assert p["sched"] == 4 and p["split"] and p["built"], p
    assert k.fused_plan(gw, "bf16")["split"]


def test_refusals_keep_their_place_and_text(k, monkeypatch):
    """A key whose kernel is not built is planned (an engine can be constructed) and refused where a launch looks it
    up: the f16 tiles have no A/B schedules."""
    ld, g = _geometry(k, 300000, "f16")  # test_gpu_f16_fused.py::test_ab_schedules_are_refused_not_substituted
    assert (g.cpl, g.T) == (8, 2)
    assert k.fused_plan(g, "f16", ld=ld, nrows_pad=256)["built"]
    monkeypatch.setenv("SART_BF16_T2_SCHED", "6")
    p = k.fused_plan(g, "f16")
    assert p["sched"] == 6 and not p["built"]
    with pytest.raises(RuntimeError, match="fused_sweep f16: schedule 6 .* is not built for f16 tiles"):
        k.fused_plan(g, "f16", ld=ld, nrows_pad=256)
    assert k.fused_plan(g, "bf16", ld=ld, nrows_pad=256)["built"]
    monkeypatch.delenv("SART_BF16_T2_SCHED")
    n1 = k.fused_geometry(65536, CUS, 6, 1, False, False)
    assert (n1.cpl, n1.T) == (4, 1)
    k.fused_set_schedule(5)
    assert not k.fused_plan(n1, "f16")["built"]
    with pytest.raises(RuntimeError, match="fused_sweep f16: schedule 5 is not built for f16 tiles"):
        k.fused_plan(n1, "f16", ld=65536, nrows_pad=256)
    assert k.fused_plan(n1, "bf16", ld=65536, nrows_pad=256)["sched"] == 5
    with pytest.raises(RuntimeError, match="fused_set_schedule: 0 .. 5"):
        k.fused_set_schedule(6)
    assert k.fused_get_schedule() == 5


def test_shape_validation(k):
    g4 = k.fused_geometry(65536, CUS, 6, 4)
    gw = k.fused_geometry_bf16_wide(65536, CUS)
    assert k.fused_plan(g4, "f32", ld=65536, nrows_pad=4096, chain_tiles=2240)["built"]
    with pytest.raises(RuntimeError, match=r"fused_sweep v6: ld must equal J \* slab"):
        k.fused_plan(g4, "f32", ld=65536 + 8192, nrows_pad=4096)
    for storage in ("bf16", "f16"):
        with pytest.raises(RuntimeError, match=rf"fused_sweep {storage}: ld must equal J \* slab"):
            k.fused_plan(gw, storage, ld=65536 + 8192, nrows_pad=4096)
        with pytest.raises(RuntimeError, match=f"fused_sweep {storage}: segment length must be a multiple of 140 tiles"):
            k.fused_plan(gw, storage, ld=65536, nrows_pad=4096, chain_tiles=100)
        with pytest.raises(RuntimeError, match=f"fused_sweep {storage}: chip-wide row groups take the wide tiles only"):
            k.fused_plan(_made(k, T=1, J=64, I=4, xl=False), storage)
        with pytest.raises(RuntimeError, match=f"fused_sweep {storage}: wide tiles need T = 4 or 2"):
            k.fused_plan(_made(k, T=1, J=8, I=32, cpl=8), storage)
        with pytest.raises(RuntimeError, match=f"fused_sweep {storage}: kw 5 ... 7 only with wide tiles"):
            k.fused_plan(_made(k, T=4, J=8, I=32, kw=7), storage)
    with pytest.raises(RuntimeError, match="fused_sweep v6: segment length must be a multiple of 140 tiles"):
        k.fused_plan(g4, "f32", ld=65536, nrows_pad=4096, chain_tiles=100)
    with pytest.raises(RuntimeError, match="fused_sweep v6: padded rows must be a multiple of 4"):
        k.fused_plan(g4, "f32", ld=65536, nrows_pad=4098)
    for kw in (5, 9):
        for T in (2, 4):
            with pytest.raises(RuntimeError, match="fused_sweep v6: 5- and 9-KiB slabs need T = 1"):
                k.fused_plan(_made(k, T=T, J=8, I=32, kw=kw), "f32")
        assert k.fused_plan(_made(k, T=1, J=8, I=32, kw=kw), "f32")["built"]
    with pytest.raises(RuntimeError, match="fused_sweep v6: lane-vectors per lane .kw. must be 5 ... 9"):
        k.fused_plan(_made(k, T=1, J=8, I=32, kw=4), "f32")
    with pytest.raises(RuntimeError, match="fused_sweep v6: XCD-local groups need .* I % 8 == 0"):
        k.fused_plan(_made(k, T=4, J=32, I=4), "f32", ld=65536, nrows_pad=4096)
    with pytest.raises(RuntimeError, match="fused_sweep v6: J \\* T > 256"):
        k.fused_plan(_made(k, T=4, J=65, I=1, xl=False), "f32", ld=65 * 2048, nrows_pad=4096)
    g3 = k.fused_geometry(65536, CUS, 3, 0)
    p3 = k.fused_plan(g3, "f32", ld=65536, nrows_pad=4096)
    assert (p3["variant"], p3["T"], p3["sched"], p3["split"], p3["threads"], p3["built"]) == (3, g3.K, -1, False, 320, True)
    with pytest.raises(RuntimeError, match=r"fused_sweep v3: ld must equal J \* 1024 \* K"):
        k.fused_plan(g3, "f32", ld=65536 + 8192, nrows_pad=4096)
    with pytest.raises(RuntimeError, match="fused_sweep: variant must be 6 or 3"):
        k.fused_plan(k.FusedGeometry(), "f32")


def test_table_sizes(k):
    """fp32 rows 40, variant 3 4, bf16 28, f16 19 keys, each for both LOG values: the 144 + 38 kernels of
    fused_sweep.hip and fused_sweep_f16.hip. The f16 keys are the bf16 ones without the A/B schedules."""
    keys = {s: [tuple(sorted(d.items())) for d in k.fused_variants(s)] for s in STORAGES}
    assert all(len(set(v)) == len(v) for v in keys.values())
    f32 = k.fused_variants("f32")
    assert (sum(d["variant"] == 6 for d in f32), sum(d["variant"] == 3 for d in f32)) == (40, 4)
    assert (len(keys["bf16"]), len(keys["f16"])) == (28, 19)
    assert 2 * (40 + 4 + 28) == 144 and 2 * 19 == 38

    def bare(d):
        return tuple(v for f, v in sorted(d.items()) if f != "storage")

    ab = {bare(d) for d in k.fused_variants("bf16")} - {bare(d) for d in k.fused_variants("f16")}
    assert {(key[4], key[1]) for key in ab} == {(6, 8), (5, 4)} and len(ab) == 9  # (sched, cpl): wide 6 x 8, narrow 5
