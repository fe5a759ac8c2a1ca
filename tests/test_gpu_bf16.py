"""bf16 storage of the RTM (opt-in precision mode): native fp32 -> bf16 rounding, the two-pass
kernels on bf16 shards against fp64 references over the stored (rounded) matrix, and the engine end to end
against the fp64 oracle of the reference GPU semantics (reference sartsolver_cuda.cpp:197-354) run on the
rounded matrix."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    from mpi_cuda_sartsolver_amd.ops import hip

    return hip()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _round_bf16(A):
    """fp32 values of the bf16 rounding (torch's conversion is round-to-nearest-even)."""
    return torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _rtm(dev, P, V, seed=0):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    rng = np.random.default_rng(seed)
    A = rng.random((P, V), dtype=np.float32)
    return _round_bf16(A), DenseRTM.from_dense(A, device=dev, storage="bf16")


def test_f32_to_bf16_matches_rne(k, dev):
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(1 << 16) * 10.0 ** rng.integers(-40, 38, 1 << 16)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                        np.nan, 1.00390625, 65504.0], dtype=np.float32)
    v[: special.size] = special
    src = torch.from_numpy(v).to(dev)
    dst = torch.empty(v.size, dtype=torch.bfloat16, device=dev)
    k.f32_to_bf16(src.data_ptr(), v.size, dst.data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    ref = src.to(torch.bfloat16)
    got = dst.view(torch.int16).cpu().numpy()
    want = ref.view(torch.int16).cpu().numpy()
    finite = ~np.isnan(v)
    np.testing.assert_array_equal(got[finite], want[finite])
    assert np.isnan(dst.float().cpu().numpy()[~finite]).all()


@pytest.mark.parametrize("P,V", [(1000, 3000), (64, 64), (2048, 4096), (777, 1025)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_forward_bf16(k, dev, P, V, epi):
    Ar, m = _rtm(dev, P, V, seed=P + V)
    assert m.A.dtype == torch.bfloat16 and m.nbytes == m.nrows_pad * m.ld * 2
    rng = np.random.default_rng(1)
    x = rng.random(V).astype(np.float32)
    gh = (rng.random(P) - 0.1).astype(np.float32)
    a = rng.random(P).astype(np.float32)
    xd = torch.zeros(m.ld, device=dev)
    xd[:V] = torch.from_numpy(x)
    ghd = torch.zeros(m.nrows_pad, device=dev)
    ghd[:P] = torch.from_numpy(gh)
    ad = torch.zeros(m.nrows_pad, device=dev)
    ad[:P] = torch.from_numpy(a)
    f = torch.zeros(m.nrows_pad, device=dev)
    w = torch.zeros(m.nrows_pad, device=dev)
    Fp = torch.zeros(k.forward_num_blocks(m.nrows_pad), dtype=torch.float64, device=dev)
    k.forward(epi, m.A.data_ptr(), m.ld, P, m.nrows_pad, xd.data_ptr(), ghd.data_ptr(), ad.data_ptr(), f.data_ptr(),
              w.data_ptr(), Fp.data_ptr(), 0, _stream(dev), True)
    torch.cuda.synchronize()
    fr = Ar.astype(np.float64) @ x.astype(np.float64)
    np.testing.assert_allclose(f[:P].cpu().numpy(), fr, rtol=2e-5)
    np.testing.assert_allclose(Fp.sum().item(), (fr.astype(np.float32).astype(np.float64) ** 2).sum(), rtol=1e-5)
    if epi == 1:
        np.testing.assert_allclose(w[:P].cpu().numpy(), a * (gh - fr), rtol=1e-4, atol=1e-3)
    if epi == 2:
        np.testing.assert_allclose(w[:P].cpu().numpy(), a * fr, rtol=2e-5)


@pytest.mark.parametrize("P,V", [(1000, 3000), (64, 64), (4096, 1024), (333, 2111)])
def test_backproject_bf16_deterministic(k, dev, P, V):
    Ar, m = _rtm(dev, P, V, seed=3)
    rng = np.random.default_rng(2)
    w = (rng.random(P) - 0.5).astype(np.float32)
    wd = torch.zeros(m.nrows_pad, device=dev)
    wd[:P] = torch.from_numpy(w)
    ns = k.backproject_num_splits(m.ld, P, 2)
    part = torch.zeros(ns * m.ld, device=dev)
    out = torch.zeros(m.ld, device=dev)
    scale = torch.ones(m.ld, device=dev)
    outs = []
    for _ in range(2):
        k.backproject(m.A.data_ptr(), m.ld, P, wd.data_ptr(), ns, part.data_ptr(), 0, _stream(dev), True)
        k.reduce_partials(part.data_ptr(), m.ld, ns, scale.data_ptr(), out.data_ptr(), 0, 0, 0, 0, _stream(dev))
        outs.append(out.clone())
    torch.cuda.synchronize()
    ref = Ar.astype(np.float64).T @ w.astype(np.float64)
    np.testing.assert_allclose(outs[0][:V].cpu().numpy(), ref, rtol=1e-4, atol=2e-4)
    assert torch.equal(outs[0], outs[1]), "back-projection must be bitwise reproducible"
    assert torch.count_nonzero(outs[0][V:]) == 0


def test_ray_sums_bf16(k, dev):
    Ar, m = _rtm(dev, 1500, 2500, seed=9)
    s = _stream(dev)
    ell = torch.zeros(m.nrows_pad, dtype=torch.float64, device=dev)
    k.rowsum_f64(m.A.data_ptr(), m.ld, m.npixel, ell.data_ptr(), s, True)
    ns = k.backproject_num_splits(m.ld, m.npixel, 2)
    part = torch.zeros(ns * m.ld, dtype=torch.float64, device=dev)
    k.colsum_f64(m.A.data_ptr(), m.ld, m.npixel, ns, part.data_ptr(), s, True)
    rho = torch.zeros(m.ld, dtype=torch.float64, device=dev)
    k.reduce_partials_f64(part.data_ptr(), m.ld, ns, rho.data_ptr(), s)
    torch.cuda.synchronize()
    A64 = Ar.astype(np.float64)
    np.testing.assert_allclose(ell[:1500].cpu().numpy(), A64.sum(1), rtol=1e-12)
    np.testing.assert_allclose(rho[:2500].cpu().numpy(), A64.sum(0), rtol=1e-12)


def test_bf16_shard_construction_paths_agree(dev):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    f = DenseRTM.synthetic(700, 1500, row_offset=300, seed=7, device=dev)
    b = DenseRTM.synthetic(700, 1500, row_offset=300, seed=7, device=dev, storage="bf16")
    c = f.to_bf16()
    assert b.A.dtype == c.A.dtype == torch.bfloat16 and b.nrows_pad == c.nrows_pad == f.nrows_pad
    assert torch.equal(b.A.view(torch.int16), c.A.view(torch.int16))
    assert torch.equal(b.A.view(torch.int16), f.A.to(torch.bfloat16).view(torch.int16))
    np.testing.assert_array_equal(b.to_host(), _round_bf16(f.to_host()))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("lap", [False, True])
def test_bf16_solver_vs_oracle(dev, log, lap, fused):
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
    from mpi_cuda_sartsolver_amd.utils.synthetic import host_problem

    A, g, _ = host_problem(2048, 4096, seed=21, saturate_fraction=0.02)
    Ar = _round_bf16(A)
    L = LaplacianCSR.grid_3d(16, 16, 16, device=dev) if lap else None
    kw = dict(max_iterations=40, conv_tolerance=0.0, beta_laplace=1e-3)
    m = DenseRTM.from_dense(A, device=dev, storage="bf16")
    s = SARTSolver(m, L, None, SolverParams(**kw), logarithmic=log, use_fused=fused, allow_zero_tolerance=True)
    assert s.use_fused == fused and (not fused or s.geom.variant == 6)
    r = s.solve(g)
    assert r.used_fused == fused, "bf16 fused exchange timed out"
    x_ref, st_ref, it_ref = sart_gpu_semantics(Ar, g, L, logarithmic=log, **kw)
    assert r.status == st_ref == -1 and r.iterations == it_ref == 40
    rel = np.linalg.norm(r.solution - x_ref) / np.linalg.norm(x_ref)
    assert rel < 2e-3
    np.testing.assert_allclose(s.ray_density64, Ar.astype(np.float64).sum(0), rtol=1e-12)


def test_bf16_synthetic_bench_problem_converges(dev):
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    prob = make_problem(4096, 8192, seed=3, device=dev, storage="bf16")
    s = SARTSolver(prob.rtm, None, None, SolverParams(max_iterations=300, conv_tolerance=1e-6))
    r = s.solve(prob.measurement)
    # g = A_bf16 x_true exactly representable by the stored matrix: SART approaches x_true
    f = s.forward_project(r.solution)
    g = prob.measurement.cpu().numpy()
    assert np.linalg.norm(f - g) / np.linalg.norm(g) < 2e-2


def test_bf16_accepted_by_multiframe(dev):
    """bf16 shards run in the multi-frame engine on the bf16 matrix cores (tests/test_gpu_multiframe_bf16.py)."""
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    m = DenseRTM.synthetic(256, 512, device=dev, storage="bf16")
    s = MultiFrameSARTSolver(m, None, None, SolverParams(max_iterations=4))
    assert s.batch_width == 16


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("log", [False, True])
def test_bf16_fused_rows_per_tile(dev, T, log):
    """bf16 variant 6 sweep with T rows per tile vs the fp64 oracle on the rounded matrix; bitwise
    reproducible from run to run, and close to the bf16 two-pass kernels (summation order only)."""
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
    from mpi_cuda_sartsolver_amd.utils.synthetic import host_problem

    A, g, _ = host_problem(1500, 32768, seed=T + 11, saturate_fraction=0.02)
    L = LaplacianCSR.grid_3d(32, 32, 32, device=dev)
    kw = dict(max_iterations=12, conv_tolerance=0.0, beta_laplace=1e-3)
    m = DenseRTM.from_dense(A, device=dev, storage="bf16")
    s = SARTSolver(m, L, None, SolverParams(**kw), logarithmic=log, allow_zero_tolerance=True, fused_variant=6,
                   fused_rows_per_tile=T)
    assert s.use_fused and s.geom.variant == 6 and s.geom.T == T
    r1 = s.solve(g)
    r2 = s.solve(g)
    assert r1.used_fused and r2.used_fused, "bf16 fused exchange timed out"
    np.testing.assert_array_equal(r1.solution, r2.solution)
    x_ref, _, _ = sart_gpu_semantics(_round_bf16(A), g, L, logarithmic=log, **kw)
    assert np.linalg.norm(r1.solution - x_ref) / np.linalg.norm(x_ref) < 2e-3
    t = SARTSolver(m, L, None, SolverParams(**kw), logarithmic=log, allow_zero_tolerance=True, use_fused=False)
    rt = t.solve(g)
    # 32768-term fp32 row dots in another summation order, amplified by 12 linear SART updates: both sit within
    # 2e-3 of the fp64 oracle, so they agree to a few 1e-3 (fp32 fused vs two-pass: test_fused_matches_two_pass)
    assert np.linalg.norm(r1.solution - rt.solution) / np.linalg.norm(rt.solution) < 3e-3


@pytest.mark.parametrize("nvox,T,J,I,kw", [(4096, 4, 1, 256, 8), (65536, 4, 16, 16, 8), (131072, 4, 32, 8, 8),
                                           (100000, 4, 28, 9, 7), (262144, 4, 64, 4, 8), (200000, 4, 49, 5, 8),
                                           (150000, 4, 42, 6, 7), (70000, 4, 18, 14, 8), (163840, 4, 40, 6, 8),
                                           (98304, 4, 28, 9, 7), (300000, 2, 42, 6, 7)])
@pytest.mark.parametrize("log", [False, True])
def test_bf16_wide_tiles(dev, monkeypatch, nvox, T, J, I, kw, log):
    """Wide bf16 tiles (16-byte loads of 8 bf16 per lane: slab 2048 kw / T columns, T = 4, or T = 2 with the 3-slot
    ring of schedule 7; kw 7 / 6 / 5 where 8 would leave CUs idle; chip-wide row groups at 150000 / 163840 / 300000
    voxels) against the narrow bf16 tiles (SART_BF16_WIDE=0) where the width allows them, else the two-pass kernels,
    and the device fp64 oracle on the stored (rounded) matrix."""
    from mpi_cuda_sartsolver_amd.models.oracle import sart_oracle_f64
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    prob = make_problem(2048, nvox, seed=nvox % 89, device=dev, saturate_fraction=0.02, storage="bf16")
    g = prob.measurement.cpu().numpy()
    p = dict(max_iterations=10, conv_tolerance=0.0)
    sw = SARTSolver(prob.rtm, None, None, SolverParams(**p), logarithmic=log, allow_zero_tolerance=True)
    assert sw.use_fused and (sw.geom.cpl, sw.geom.T, sw.geom.J, sw.geom.I, sw.geom.kw) == (8, T, J, I, kw)
    rw = sw.solve(g)
    assert rw.used_fused and rw.fallbacks == 0
    np.testing.assert_array_equal(rw.solution, sw.solve(g).solution)  # bitwise reproducible
    del sw
    monkeypatch.setenv("SART_BF16_WIDE", "0")
    sn = SARTSolver(prob.rtm, None, None, SolverParams(**p), logarithmic=log, allow_zero_tolerance=True)
    if not sn.use_fused:  # no narrow-tile geometry at this padded width: the two-pass kernels set the scale
        del sn
        sn = SARTSolver(prob.rtm, None, None, SolverParams(**p), logarithmic=log, allow_zero_tolerance=True,
                        use_fused=False)
    else:
        assert sn.geom.cpl == 4
    rn = sn.solve(g)
    del sn
    x64 = sart_oracle_f64(prob.rtm, g, 10, logarithmic=log)
    ew = np.linalg.norm(rw.solution - x64) / np.linalg.norm(x64)
    en = np.linalg.norm(rn.solution - x64) / np.linalg.norm(x64)
    # summation-order differences only (measured 1.27x at 4096 columns, <= 1.1x at >= 64k)
    assert ew <= 1.5 * en + 1e-7, (ew, en)


@pytest.mark.parametrize("log", [False, True])
def test_bf16_wide_t2_schedules_agree(dev, monkeypatch, log):
    """Wide bf16 tiles at T = 2: schedule 7 (4-step lag, the default) and schedule 6 (3-step lag,
    SART_BF16_T2_SCHED=6) run the same arithmetic in the same order, so their iterates are bitwise equal; both are
    fused (no fallback) and match the device fp64 oracle on the stored matrix."""
    from mpi_cuda_sartsolver_amd.models.oracle import sart_oracle_f64
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    monkeypatch.setenv("SART_BF16_XL", "1")  # XCD-local groups: 262144 voxels at T = 2 (by default chip-wide at T = 4)
    prob = make_problem(4096, 262144, seed=7, device=dev, saturate_fraction=0.02, storage="bf16")
    g = prob.measurement.cpu().numpy()
    p = SolverParams(max_iterations=8, conv_tolerance=0.0)
    out = {}
    for sched in ("7", "6"):
        monkeypatch.setenv("SART_BF16_T2_SCHED", sched)
        s = SARTSolver(prob.rtm, None, None, p, logarithmic=log, allow_zero_tolerance=True)
        assert s.use_fused and (s.geom.cpl, s.geom.T) == (8, 2)
        planned = s.k.fused_plan(s.geom, "bf16")["sched"]
        r = s.solve(g)
        assert r.used_fused and r.fallbacks == 0
        assert s.k.fused_last_schedule() == planned == int(sched)
        out[sched] = r.solution
        del s
    np.testing.assert_array_equal(out["7"], out["6"])
    # fp32 drift of 8 iterations on a 262144-wide random matrix is ~7e-3 for any summation order: compare with
    # the bf16 two-pass kernels' distance to the oracle, not with a fixed bound
    t = SARTSolver(prob.rtm, None, None, p, logarithmic=log, allow_zero_tolerance=True, use_fused=False)
    r2 = t.solve(g)
    x64 = sart_oracle_f64(prob.rtm, g, 8, logarithmic=log)
    e7 = np.linalg.norm(out["7"] - x64) / np.linalg.norm(x64)
    e2 = np.linalg.norm(r2.solution - x64) / np.linalg.norm(x64)
    assert e7 <= max(1.5 * e2, 1e-5), (e7, e2)
