"""The fused single-pass sweep on row-scaled f16 shards (opt-in: ``SARTSolver(..., f16_fused=True)`` /
``EngineConfig.f16_fused`` / ``--rtm_f16_fused``): variant 6 on f16 tiles (csrc/kernels/fused_sweep_f16.hip) against
fp64 oracles over the dequantised matrix H / s_p, against the two-pass f16 kernels at every planned geometry, and the
native driver end to end. Every solve is checked to have run fused without a fallback and to repeat bit for bit (the
sweep's sums have a fixed order). Without the opt-in f16 shards keep the two-pass kernels (tests/test_gpu_f16.py)."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FACTOR, SLACK = 1.0, 2e-8  # the bounds of tests/test_gpu_realistic.py and tests/test_gpu_f16.py


@pytest.fixture(scope="module")
def k():
    from mpi_cuda_sartsolver_amd.ops import hip

    return hip()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cache():
    return {}  # references shared between the cases of a parametrised test (computed once, never modified)


def _quantise(A):
    from mpi_cuda_sartsolver_amd.utils.f16rows import quantise_rows_f16

    return quantise_rows_f16(A)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _solver(m, L=None, *, log=False, **kw):
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams

    p = {x: kw.pop(x) for x in list(kw) if x in ("max_iterations", "beta_laplace", "ray_length_threshold",
                                                  "ray_density_threshold")}
    return SARTSolver(m, L, None, SolverParams(conv_tolerance=0.0, **p), logarithmic=log, allow_zero_tolerance=True,
                      **kw)


def _solve_fused_twice(s, g, x0=None):
    """One solve on the fused sweep, checked fused / no fallback / bitwise repeatable."""
    assert s.use_fused
    r = s.solve(g, x0)
    assert r.used_fused and r.fallbacks == 0
    r2 = s.solve(g, x0)
    assert r2.used_fused and r2.fallbacks == 0
    np.testing.assert_array_equal(r.solution, r2.solution)
    return r


# ---------------------------------------------------------------------------------------------- 1. the opt-in


def test_opt_in_constructs_and_runs_fused(k, dev):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.utils.synthetic import host_problem

    assert k.EngineConfig().f16_fused is False
    A, g, _ = host_problem(300, 4096, seed=5)
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    s = _solver(m, max_iterations=3, f16_fused=True)  # use_fused=None resolves to the opt-in
    assert s.use_fused and s.geom is not None and s.geom.variant == 6
    r = _solve_fused_twice(s, g)
    assert r.iterations == 3 and r.fused_variant == 6
    assert _solver(m, max_iterations=3, f16_fused=True, use_fused=True).use_fused
    assert not _solver(m, max_iterations=3, f16_fused=True, use_fused=False).use_fused
    assert not _solver(m, max_iterations=3).use_fused  # the default stays two-pass
    with pytest.raises(ValueError, match="fused f16 sweep is not built yet"):
        _solver(m, max_iterations=3, use_fused=True)
    for storage in ("fp32", "bf16"):
        other = DenseRTM.from_dense(A, device=dev, storage=storage)
        with pytest.raises(ValueError, match="f16_fused applies to row-scaled f16 shards"):
            _solver(other, max_iterations=3, f16_fused=True)


def test_engine_config_rules(k, dev):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    m = DenseRTM.synthetic(128, 4096, device=dev, storage="f16")
    f = DenseRTM.synthetic(128, 4096, device=dev)
    comm = k.local_comm()

    def cfg(**kw):
        c = k.EngineConfig()
        c.rtm_f16, c.use_fused, c.row_scale = True, False, m.row_scale.data_ptr()
        for name, v in kw.items():
            setattr(c, name, v)
        return c

    args = (0, m.A.data_ptr(), m.npixel, m.nrows_pad, m.nvoxel, m.ld, comm)
    assert k.Engine(*args, cfg(use_fused=True, f16_fused=True)).use_fused
    assert not k.Engine(*args, cfg(f16_fused=True)).use_fused  # the opt-in alone does not switch the sweep on
    with pytest.raises(ValueError, match="fused f16 sweep is not built yet"):
        k.Engine(*args, cfg(use_fused=True))
    with pytest.raises(ValueError, match="f16_fused applies to row-scaled f16 shards"):
        k.Engine(0, f.A.data_ptr(), f.npixel, f.nrows_pad, f.nvoxel, f.ld, comm,
                 cfg(rtm_f16=False, row_scale=0, f16_fused=True))


# ---------------------------------------------------------------------------------------------- 2. ray-traced fixture


@pytest.fixture(scope="module")
def realistic():
    from mpi_cuda_sartsolver_amd.utils.raytrace import phantom, raytraced_rtm

    A, _ = raytraced_rtm(grid=(16, 16, 16))
    rng = np.random.default_rng(3)
    X = np.stack([phantom((16, 16, 16), t=float(t)) for t in range(128)])
    G = X @ A.T.astype(np.float64)
    G[rng.random(G.shape) < 0.02] = -1.0  # saturated pixels (the fixture of tests/test_gpu_realistic.py)
    return A, G, _quantise(A)


@pytest.fixture(scope="module")
def lap(dev):
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR

    return LaplacianCSR.grid_3d(16, 16, 16, device=dev)


def _errors(x, A, g, L, *, log, iters, beta):
    """(ours, fp32 emulation) errors against the fp64 oracle, all three on the same matrix A."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_fp32_emulation, sart_gpu_semantics

    kw = dict(logarithmic=log, max_iterations=iters, beta_laplace=beta)
    x64, _, _ = sart_gpu_semantics(A, g, L, conv_tolerance=0.0, **kw)
    e32 = max(_rel(sart_fp32_emulation(A, g, L, order=o, **kw)[0], x64) for o in ("blas", "reference"))
    return _rel(x, x64), e32


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("with_lap", [False, True])
def test_fused_on_the_raytraced_matrix(dev, realistic, lap, log, with_lap):
    """2048 x 4096 ray-traced model, 40 updates: no further from the fp64 oracle on the dequantised matrix than an
    fp32 evaluation on that matrix (the bound the fp32 fused sweep meets here; after the exact widening the f16
    sweep's arithmetic is fp32 too).

    In logarithmic mode the update multiplies by (O + eps) / (Fv + eps) with O = A^T (a g) summed once per frame and
    Fv = A^T (a f) by every sweep. The engine therefore has the f16 sweep sum O itself (one observed sweep in the
    frame set-up), so that both sums run in the same order and their roundings cancel in the ratio as they do on
    the two-pass kernels; with O from the two-pass back-projection the sweep measured 1.09x / 1.12x the emulation's
    error here (without / with the Laplacian), over the bound; with its own O 0.87x - 0.92x, linear 0.87x - 0.93x."""
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, G, q = realistic
    L = lap if with_lap else None
    beta = 1e-3
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    s = _solver(m, L, log=log, max_iterations=40, beta_laplace=beta, f16_fused=True)
    assert s.use_fused and s.geom.cpl == 8
    for f in (0, 5):
        r = _solve_fused_twice(s, G[f])
        assert r.iterations == 40
        e, e32 = _errors(r.solution, q.dequantised, G[f], L, log=log, iters=40, beta=beta)
        print(f"f16 fused log={log} lap={with_lap} frame {f}: {e:.3e} (fp32 emulation {e32:.3e}, "
              f"ratio {e / e32:.3f})")
        assert e <= FACTOR * e32 + SLACK, (f, e, e32)


# ---------------------------------------------------------------------------------------------- 3. row scales


def _decades(P, V, seed):
    """rng.random times per-row factors over 15 decades in random order (as tests/test_gpu_f16.py)."""
    rng = np.random.default_rng(seed)
    fac = rng.permutation(np.logspace(-12, 3, P)).astype(np.float32)
    return rng.random((P, V), dtype=np.float32) * fac[:, None], fac.astype(np.float64)


THR = 1e-13  # ray-length threshold of the 15-decade matrix: below its smallest row sum (~2048 x 1e-12)


@pytest.fixture(scope="module")
def decades():
    A, fac = _decades(777, 4096, seed=21)
    q = _quantise(A)
    rng = np.random.default_rng(4)
    g = q.dequantised.astype(np.float64) @ rng.random(4096)
    return A, q, g


@pytest.mark.parametrize("log", [False, True])
def test_row_scales_over_fifteen_decades(dev, decades, log):
    """One update, element by element against the fp64 oracle on the dequantised matrix. The rows' scales span 50
    binary orders, so a 1 / s_p forgotten or applied twice -- in the row dot or in the weight -- is off by orders of
    magnitude in every row but a few."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, q, g = decades
    ell = q.dequantised.astype(np.float64).sum(1).astype(np.float32)
    assert np.all(ell > np.float32(THR)) and np.all(g > 0), "no row may be masked"
    assert np.log2(q.scales.max() / q.scales.min()) > 45
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    s = _solver(m, log=log, max_iterations=1, ray_length_threshold=THR, f16_fused=True)
    r = _solve_fused_twice(s, g)
    assert r.iterations == 1 and not r.nonfinite
    x64, _, _ = sart_gpu_semantics(q.dequantised, g, None, logarithmic=log, max_iterations=1, conv_tolerance=0.0,
                                   ray_length_threshold=THR)
    err = np.abs(r.solution - x64).max() / np.abs(x64).max()
    print(f"f16 fused, 15 decades, log={log}: max |x - x64| / max |x64| = {err:.3e}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("log", [False, True])
def test_nan_row_stops_the_solve_as_on_the_two_pass_kernels(dev, decades, log):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, _, g = decades
    B = A.copy()
    B[100, 3] = np.nan  # one NaN in one row (stored as the quiet NaN 0x7e00)
    m = DenseRTM.from_dense(B, device=dev, storage="f16")
    kw = dict(log=log, max_iterations=5, ray_length_threshold=THR)
    sf = _solver(m, f16_fused=True, **kw)
    assert sf.use_fused
    rf = sf.solve(g)
    assert rf.used_fused and rf.fallbacks == 0
    rt = _solver(m, **kw).solve(g)
    assert not rt.used_fused
    assert rt.nonfinite, "the two-pass f16 kernels stop on the NaN row"
    assert (rf.nonfinite, rf.status, rf.iterations) == (rt.nonfinite, rt.status, rt.iterations)


# ---------------------------------------------------------------------------------------------- 4. stored subnormals


@pytest.fixture(scope="module")
def subnormal_case():
    """64 x 4096: row p holds its maximum 2^18 in column p and 2^-36 ... 2^-30 of it everywhere else, which the format
    stores as f16 subnormals. The start value is tiny in the 64 maximum columns and large elsewhere, so the
    subnormal entries carry most of every row dot; 2^18 puts the measurement's maximum (the solver's normalisation)
    near one, so that the start value below survives the solvers' floor of 1e-7 on the normalised iterate."""
    P, V = 64, 4096
    rng = np.random.default_rng(8)
    M = np.float32(2.0 ** 18)
    A = (M * 2.0 ** rng.uniform(-36, -30, (P, V))).astype(np.float32)
    A[np.arange(P), np.arange(P)] = M
    q = _quantise(A)
    off = ~np.eye(P, V, dtype=bool)
    h = np.abs(q.bits.view(np.float16).astype(np.float32))
    assert np.all((h[off] > 0) & (h[off] < 2.0 ** -14)), "every other entry is stored as a non-zero f16 subnormal"
    assert np.all(h[~off] >= 2.0 ** 13)
    D = q.dequantised.astype(np.float64)
    Z = np.where(off, 0.0, D)  # the matrix a flush of subnormal inputs would see
    xh = np.full(V, 4.0)
    xh[:P] = 4e-7
    g = D @ (xh * (1.0 + 0.5 * rng.random(V)))
    # 0.6 xh after the solver's normalisation by max g (about 1.35): the normalised measurement is close to 1 in every
    # row and the start value's row dots close to 0.65, so the first update's weights are of order one
    x0 = 0.6 * xh * g.max()
    carried = ((D - Z) @ xh) / (D @ xh)
    assert carried.min() > 0.5, "the subnormal entries carry more than half of every row dot"
    return A, q, D, Z, g, x0


@pytest.mark.parametrize("log", [False, True])
def test_stored_subnormals_count(dev, subnormal_case, log):
    """The mixed-precision FMAs widen f16 subnormals exactly: one update matches the fp64 oracle on the dequantised
    matrix element by element (the bound of the 15-decade case), and is not the update of the matrix with the
    subnormal entries zeroed. Where the two oracles are at least a quarter apart (the 64 maximum columns, whose
    updates are formed from their rows' dots with weights of order one; the other voxels' updates are weighted by
    entries 2^-30 of a row sum and hardly move), the result must sit within 1e-3 of the first, relative per element:
    fp32 sums of 4096 terms and one subtraction that cancels about two thirds lose at most a few 1e-6 there, and a
    flush would move these voxels by 25 % or more."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, q, D, Z, g, x0 = subnormal_case
    kw = dict(logarithmic=log, max_iterations=1, conv_tolerance=0.0, x_prev=x0)
    x64, _, _ = sart_gpu_semantics(D, g, None, **kw)
    xz, _, _ = sart_gpu_semantics(Z, g, None, **kw)
    apart = np.abs(x64 - xz) >= 0.25 * np.abs(x64)
    assert apart[:64].all(), "the fixture separates the two oracles"
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    assert m.flushed_count == q.flushed == 64 * 4095
    s = _solver(m, log=log, max_iterations=1, f16_fused=True)
    r = _solve_fused_twice(s, g, x0)
    assert r.iterations == 1 and not r.nonfinite
    err = np.abs(r.solution - x64).max() / np.abs(x64).max()
    rel = (np.abs(r.solution - x64)[apart] / np.abs(x64)[apart]).max()
    far = (np.abs(r.solution - xz)[apart] / np.abs(x64)[apart]).min()
    print(f"f16 fused, subnormal rows, log={log}: max |x - x64| / max |x64| = {err:.3e}; where the zeroed oracle "
          f"differs: within {rel:.3e} of x64, at least {far:.3e} from it")
    assert err <= 1e-5, err
    assert rel <= 1e-3, rel
    assert far >= 0.24, far


# ---------------------------------------------------------------------------------------------- 5. geometries


def _two_pass_error(cache, key, prob, g, log, iters=10):
    """(fp64 oracle on the stored matrix, error of the two-pass f16 kernels against it), once per problem."""
    from mpi_cuda_sartsolver_amd.models.oracle import sart_oracle_f64

    if key not in cache:
        x64 = sart_oracle_f64(prob.rtm, g, iters, logarithmic=log)
        rn = _solver(prob.rtm, log=log, max_iterations=iters).solve(g)
        assert not rn.used_fused
        cache[key] = (x64, _rel(rn.solution, x64))
    return cache[key]


@pytest.mark.parametrize("nvox,T,J,I,kw", [(4096, 4, 1, 256, 8), (65536, 4, 16, 16, 8), (100000, 4, 28, 9, 7),
                                           (150000, 4, 42, 6, 7), (300000, 2, 42, 6, 7)])
@pytest.mark.parametrize("log", [False, True])
def test_f16_wide_tiles(dev, cache, nvox, T, J, I, kw, log):
    """Wide f16 tiles at the geometry the bf16 sweep plans for the same width (no exchange; XCD-local exchange;
    narrower slabs; chip-wide row groups; T = 2 on schedule 7) against the two-pass f16 kernels: both within
    summation order of the device fp64 oracle on the stored matrix (the bound of test_bf16_wide_tiles)."""
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    prob = make_problem(2048, nvox, seed=nvox % 89, device=dev, saturate_fraction=0.02, storage="f16")
    g = prob.measurement.cpu().numpy()
    sw = _solver(prob.rtm, log=log, max_iterations=10, f16_fused=True)
    assert sw.use_fused and (sw.geom.cpl, sw.geom.T, sw.geom.J, sw.geom.I, sw.geom.kw) == (8, T, J, I, kw)
    rw = _solve_fused_twice(sw, g)
    del sw
    x64, en = _two_pass_error(cache, ("wide", nvox, log), prob, g, log)
    ew = _rel(rw.solution, x64)
    print(f"f16 fused wide {nvox} log={log}: {ew:.3e} (two-pass {en:.3e}, ratio {ew / en:.3f})")
    assert ew <= 1.5 * en + 1e-7, (ew, en)


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("log", [False, True])
def test_f16_narrow_tiles_rows_per_tile(dev, cache, monkeypatch, T, log):
    """Narrow f16 tiles (8-byte loads) at 1, 2 and 4 rows per tile; 1500 rows pad to 1536 (padding rows with
    s_p = 1 and zero weight)."""
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    monkeypatch.setenv("SART_BF16_WIDE", "0")  # (T = 4 would otherwise plan the wide tiles)
    prob = make_problem(1500, 32768, seed=13, device=dev, saturate_fraction=0.02, storage="f16")
    assert prob.rtm.nrows_pad == 1536
    g = prob.measurement.cpu().numpy()
    s = _solver(prob.rtm, log=log, max_iterations=10, f16_fused=True, fused_variant=6, fused_rows_per_tile=T)
    assert s.use_fused and (s.geom.variant, s.geom.cpl, s.geom.T, s.geom.kw) == (6, 4, T, 8)
    r = _solve_fused_twice(s, g)
    del s
    x64, en = _two_pass_error(cache, ("narrow", 32768, log), prob, g, log)
    ew = _rel(r.solution, x64)
    print(f"f16 fused narrow T={T} log={log}: {ew:.3e} (two-pass {en:.3e}, ratio {ew / en:.3f})")
    assert ew <= 1.5 * en + 1e-7, (ew, en)


@pytest.mark.parametrize("log", [False, True])
def test_f16_narrow_tiles_at_the_headline_width(dev, cache, monkeypatch, log):
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    monkeypatch.setenv("SART_BF16_WIDE", "0")
    prob = make_problem(2048, 65536, seed=65536 % 89, device=dev, saturate_fraction=0.02, storage="f16")
    g = prob.measurement.cpu().numpy()
    s = _solver(prob.rtm, log=log, max_iterations=10, f16_fused=True)
    assert s.use_fused and s.geom.cpl == 4
    r = _solve_fused_twice(s, g)
    del s
    x64, en = _two_pass_error(cache, ("wide", 65536, log), prob, g, log)  # (the problem of test_f16_wide_tiles)
    ew = _rel(r.solution, x64)
    print(f"f16 fused narrow 65536 log={log}: {ew:.3e} (two-pass {en:.3e}, ratio {ew / en:.3f})")
    assert ew <= 1.5 * en + 1e-7, (ew, en)


def test_ab_schedules_are_refused_not_substituted(dev, monkeypatch):
    """The bf16 sweep's A/B schedules are not built for f16 tiles: asking for one is an error at the first sweep, not
    a silent run of another kernel (no GPU work is started for it)."""
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    prob = make_problem(256, 300000, seed=3, device=dev, storage="f16")
    g = prob.measurement.cpu().numpy()
    monkeypatch.setenv("SART_BF16_T2_SCHED", "6")
    s = _solver(prob.rtm, max_iterations=2, f16_fused=True)
    assert s.use_fused and (s.geom.cpl, s.geom.T) == (8, 2)
    with pytest.raises(RuntimeError, match="schedule 6 .* is not built for f16 tiles"):
        s.solve(g)


# ---------------------------------------------------------------------------------------------- 6. CLI


def test_cli_rtm_f16_fused(tmp_path, capfd, monkeypatch):
    """sartsolver --rtm_f16 --rtm_f16_fused frame by frame on HDF5 files of the ray-traced model. The driver keeps the
    fused sweep for shards of at least SART_FUSED_MIN_MB (default 128) and this 2048 x 4096 f16 shard has 16 MB, so
    the plain run reports the two-pass kernels; the fused CLI path is then run on the same case with the driver's
    threshold variable set to 0 (the smallest case that plans fused: one slab, J = 1), and every frame is held
    against the oracle of the same warm-start chain on the emulation's dequantised matrix."""
    from mpi_cuda_sartsolver_amd import cli
    from mpi_cuda_sartsolver_amd.io.fixtures import make_case

    from test_cli_e2e import chain_errors

    case = make_case(str(tmp_path / "c"), shapes=((32, 32), (32, 32)), grid=(16, 16, 16), raytraced=True,
                     sparse_cameras=("cam_b",), laplacian=True, nframes=4, saturate=0.02, mask_fraction=0.1)
    q = _quantise(case.A)
    out, prof = str(tmp_path / "out.h5"), str(tmp_path / "prof.jsonl")
    argv = ["--rtm_f16", "--rtm_f16_fused", "-m", "40", "-c", "1e-7", "-l", case.laplacian_file, "-b", "1e-3",
            "-o", out, "--profile", prof] + case.files
    monkeypatch.delenv("SART_FUSED_MIN_MB", raising=False)
    assert cli.main(argv) == 0
    assert capfd.readouterr().out.count("Processed in:") == 4
    load = [json.loads(ln) for ln in open(prof)][0]
    assert load["load"] and load["rtm_storage"] == "f16" and load["solver_path"] == "two-pass"

    monkeypatch.setenv("SART_FUSED_MIN_MB", "0")
    assert cli.main(argv) == 0
    assert capfd.readouterr().out.count("Processed in:") == 4
    load = [json.loads(ln) for ln in open(prof)][0]
    assert load["load"] and load["rtm_storage"] == "f16" and load["f16_flushed"] == q.flushed
    assert load["solver_path"] == "fused"  # what a fused bf16 run reports
    e, e32 = chain_errors(case, out, warm=True, A=q.dequantised, orders=("blas", "reference"))
    print("cli --rtm_f16 --rtm_f16_fused", e, e32, e / e32)
    assert np.all(e <= FACTOR * e32 + SLACK), (e, e32)

    # --two_pass wins over the opt-in; the opt-in needs --rtm_f16
    assert cli.main(["--two_pass"] + argv) == 0
    capfd.readouterr()
    assert [json.loads(ln) for ln in open(prof)][0]["solver_path"] == "two-pass"
    assert cli.main(["--rtm_f16_fused", "-o", out] + case.files) == 1
    assert "Argument rtm_f16_fused needs rtm_f16." in capfd.readouterr().err
