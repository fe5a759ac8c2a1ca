"""Row-scaled f16 storage of the RTM (opt-in, ``DenseRTM(storage="f16")`` / ``--rtm_f16``): the device conversion
kernel bit for bit against its NumPy definition (utils/f16rows.py), the two-pass kernels on f16 shards against fp64
references over the dequantised matrix H / s_p, the single-frame engine on the ray-traced fixture at the fp32
two-pass bound, and the native driver end to end."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FACTOR, MF_FACTOR, SLACK = 1.0, 1.03, 2e-8  # the bounds of tests/test_gpu_realistic.py


@pytest.fixture(scope="module")
def k():
    from mpi_cuda_sartsolver_amd.ops import hip

    return hip()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _quantise(A):
    from mpi_cuda_sartsolver_amd.utils.f16rows import quantise_rows_f16

    return quantise_rows_f16(A)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _special_rows(V):
    """all-zero; maximum exactly 2^k; maximum nextafter(2^k, 0); entries from 1e-30 to 1e3; one NaN and one inf."""
    rng = np.random.default_rng(V)
    R = np.zeros((5, V), dtype=np.float32)
    R[1] = rng.random(V, dtype=np.float32) * 2.0 ** -8
    R[1, V // 2] = 2.0 ** -7
    R[1, 1] = -(2.0 ** -7)
    R[2] = rng.random(V, dtype=np.float32) * 31.0
    R[2, V - 1] = np.nextafter(np.float32(32.0), np.float32(0))
    R[3] = (10.0 ** rng.uniform(-30, 3, V)).astype(np.float32) * rng.choice([-1.0, 1.0], V).astype(np.float32)
    R[3, 0], R[3, 5 % V] = 1e3, 1e-30
    R[4] = rng.random(V, dtype=np.float32) * 1e-5
    R[4, 3], R[4, V - 2] = np.nan, np.inf
    return R


def _decades(P, V, seed):
    """rng.random times per-row factors over 15 decades in random order: a range one shard-wide scale could not hold."""
    rng = np.random.default_rng(seed)
    fac = rng.permutation(np.logspace(-12, 3, P)).astype(np.float32)
    return rng.random((P, V), dtype=np.float32) * fac[:, None], fac.astype(np.float64)


# ---------------------------------------------------------------------------------------------- 1. conversion


@pytest.mark.parametrize("n,ld,V", [(64, 64, 64), (5, 1088, 1025), (777, 1088, 1025)])
def test_conversion_is_bitwise_the_emulation(k, dev, n, ld, V):
    A, _ = _decades(n, V, seed=n + V)
    sp = _special_rows(V)
    A[: min(n, 5)] = sp[: min(n, 5)]
    if n > 5:
        A[n - 5:] = sp[::-1]
    q = _quantise(A)
    src = np.full((n, ld), 7e30, dtype=np.float32)  # columns >= nvoxel: ignored by the maximum, stored as zero
    src[:, :V] = A
    srcd = torch.from_numpy(src).to(dev)
    dst = torch.full((n, ld), 0x3C00, dtype=torch.int16, device=dev)
    sc = torch.zeros(2 * n, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    for _ in range(2):  # the counters accumulate over launches (one pair per shard)
        k.f32_to_f16_rows(srcd.data_ptr(), n, ld, V, dst.data_ptr(), sc.data_ptr(), sc[n:].data_ptr(), cnt.data_ptr(),
                          _stream(dev))
    torch.cuda.synchronize()
    got = _bits(dst)
    np.testing.assert_array_equal(got[:, :V], q.bits)
    assert not got[:, V:].any()
    np.testing.assert_array_equal(sc[:n].cpu().numpy().view(np.uint32), q.scales.view(np.uint32))
    np.testing.assert_array_equal(sc[n:].cpu().numpy().view(np.uint32), (np.float32(1) / q.scales).view(np.uint32))
    fin = np.isfinite(A)
    assert cnt.cpu().tolist() == [2 * q.flushed, 2 * int(np.count_nonzero(fin & (A != 0)))]
    assert q.flushed > 0  # (the 1e-30 .. 1e3 row has entries in the subnormal range and below it)
    # without counters
    k.f32_to_f16_rows(srcd.data_ptr(), n, ld, V, dst.data_ptr(), sc.data_ptr(), sc[n:].data_ptr(), 0, _stream(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(dst)[:, :V], q.bits)


def test_construction_paths_agree_bitwise(dev):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    f = DenseRTM.synthetic(700, 1500, row_offset=300, seed=7, device=dev, lo=0.0, hi=1.0)
    a = DenseRTM.synthetic(700, 1500, row_offset=300, seed=7, device=dev, storage="f16")
    b = f.to_f16()
    A = f.to_host()
    c = DenseRTM.from_dense(A, row_offset=300, device=dev, storage="f16")
    d = DenseRTM(700, 1500, row_offset=300, device=dev, storage="f16")
    d.A.zero_()
    pinned = torch.from_numpy(A).pin_memory()
    d.fill_rows(0, pinned[:333])
    d.fill_rows(333, pinned[333:])
    q = _quantise(A)
    for m in (a, b, c, d):
        assert m.is_f16 and not m.is_bf16 and m.A.dtype == torch.float16 and m.nbytes == m.nrows_pad * m.ld * 2
        assert m.nrows_pad == f.nrows_pad
        np.testing.assert_array_equal(_bits(m.A)[:700, :1500], q.bits)
        assert not _bits(m.A)[700:].any() and not _bits(m.A)[:, 1500:].any()
        rs = m.row_scale.cpu().numpy()
        np.testing.assert_array_equal(rs[:700], q.scales)
        np.testing.assert_array_equal(rs[m.nrows_pad: m.nrows_pad + 700], np.float32(1) / q.scales)
        assert np.all(rs[700: m.nrows_pad] == 1) and np.all(rs[m.nrows_pad + 700:] == 1)  # padding rows
        np.testing.assert_array_equal(m.dequantised().cpu().numpy(), q.dequantised)
        np.testing.assert_array_equal(m.to_host(), q.dequantised)
        assert m.flushed_count == q.flushed and m.nonzero_count == int(np.count_nonzero(A))
    with pytest.raises(ValueError, match="row shards"):
        DenseRTM(64, 64, device=dev, storage="f16", col_offset=0, nvoxel_total=128)
    with pytest.raises(ValueError, match="'fp32', 'bf16' or 'f16'"):
        DenseRTM(64, 64, device=dev, storage="fp16")


# ---------------------------------------------------------------------------------------------- 2. two-pass kernels


def _rtm(dev, P, V, seed):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, fac = _decades(P, V, seed)
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    return _quantise(A), m, fac


def _rinv(m):
    return m.row_scale[m.nrows_pad:]


@pytest.mark.parametrize("P,V", [(1000, 3000), (64, 64), (2048, 4096), (777, 1025)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_forward_f16(k, dev, P, V, epi):
    """f = (1 / s_p) dot(H_p, x) against fp64 over the dequantised matrix, at the tolerances of the bf16 tests with
    their absolute term relative to the row's factor; the weight written for the back-projection carries 1 / s_p."""
    q, m, fac = _rtm(dev, P, V, seed=P + V)
    rng = np.random.default_rng(1)
    x = rng.random(V).astype(np.float32)
    gh = ((rng.random(P) - 0.1) * fac).astype(np.float32)
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
              w.data_ptr(), Fp.data_ptr(), 0, _stream(dev), False, True, _rinv(m).data_ptr())
    torch.cuda.synchronize()
    A64 = q.dequantised.astype(np.float64)
    fr = A64 @ x.astype(np.float64)
    np.testing.assert_allclose(f[:P].cpu().numpy(), fr, rtol=2e-5)
    np.testing.assert_allclose(Fp.sum().item(), (fr.astype(np.float32).astype(np.float64) ** 2).sum(), rtol=1e-5)
    ri = (1.0 / q.scales.astype(np.float64))
    got = w[:P].cpu().numpy().astype(np.float64)
    if epi == 1:
        ref = ri * (a.astype(np.float64) * (gh.astype(np.float64) - fr))
        assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-3 * fac * ri), np.abs(got - ref).max()
    if epi == 2:
        np.testing.assert_allclose(got, ri * (a.astype(np.float64) * fr), rtol=2e-5)
    with pytest.raises(RuntimeError, match="needs its row scales"):
        k.forward(epi, m.A.data_ptr(), m.ld, P, m.nrows_pad, xd.data_ptr(), ghd.data_ptr(), ad.data_ptr(),
                  f.data_ptr(), w.data_ptr(), Fp.data_ptr(), 0, _stream(dev), False, True, 0)


@pytest.mark.parametrize("P,V", [(1000, 3000), (64, 64), (2048, 4096), (777, 1025), (333, 2111)])
def test_backproject_f16_deterministic(k, dev, P, V):
    """sum_p H[p][v] w'[p] with w' = w / s_p, i.e. A^T w over the dequantised matrix. w is taken per unit of the row's
    factor, so every row contributes terms of order one and the bf16 test's tolerances (rtol 1e-4, atol 2e-4) apply
    as they stand; a lost row scale would be off by decades."""
    q, m, fac = _rtm(dev, P, V, seed=3)
    rng = np.random.default_rng(2)
    w = ((rng.random(P) - 0.5) / fac).astype(np.float32)
    wd = torch.zeros(m.nrows_pad, device=dev)
    wd[:P] = torch.from_numpy(w)
    k.scale_rows(wd.data_ptr(), _rinv(m).data_ptr(), m.nrows_pad, _stream(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(wd[:P].cpu().numpy(), w * (np.float32(1) / q.scales))  # exact: powers of two
    ns = k.backproject_num_splits(m.ld, P, 2)
    part = torch.zeros(ns * m.ld, device=dev)
    out = torch.zeros(m.ld, device=dev)
    scale = torch.ones(m.ld, device=dev)
    outs = []
    for _ in range(2):
        k.backproject(m.A.data_ptr(), m.ld, P, wd.data_ptr(), ns, part.data_ptr(), 0, _stream(dev), False, True)
        k.reduce_partials(part.data_ptr(), m.ld, ns, scale.data_ptr(), out.data_ptr(), 0, 0, 0, 0, _stream(dev))
        outs.append(out.clone())
    torch.cuda.synchronize()
    ref = q.dequantised.astype(np.float64).T @ w.astype(np.float64)
    np.testing.assert_allclose(outs[0][:V].cpu().numpy(), ref, rtol=1e-4, atol=2e-4)
    assert torch.equal(outs[0], outs[1]), "back-projection must be bitwise reproducible"
    assert torch.count_nonzero(outs[0][V:]) == 0


def test_ray_sums_f16(k, dev):
    q, m, _ = _rtm(dev, 1500, 2500, seed=9)
    s = _stream(dev)
    ell = torch.zeros(m.nrows_pad, dtype=torch.float64, device=dev)
    k.rowsum_f64(m.A.data_ptr(), m.ld, m.npixel, ell.data_ptr(), s, False, True, _rinv(m).data_ptr())
    ns = k.backproject_num_splits(m.ld, m.npixel, 2)
    part = torch.zeros(ns * m.ld, dtype=torch.float64, device=dev)
    k.colsum_f64(m.A.data_ptr(), m.ld, m.npixel, ns, part.data_ptr(), s, False, True, _rinv(m).data_ptr())
    rho = torch.zeros(m.ld, dtype=torch.float64, device=dev)
    k.reduce_partials_f64(part.data_ptr(), m.ld, ns, rho.data_ptr(), s)
    torch.cuda.synchronize()
    A64 = q.dequantised.astype(np.float64)
    np.testing.assert_allclose(ell[:1500].cpu().numpy(), A64.sum(1), rtol=1e-12)
    np.testing.assert_allclose(rho[:2500].cpu().numpy(), A64.sum(0), rtol=1e-12)
    assert torch.count_nonzero(rho[2500:]) == 0


# ---------------------------------------------------------------------------------------------- 3. SARTSolver


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


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _errors(x, A, g, L, *, log, iters, beta):
    """(ours, fp32 emulation) errors against the fp64 oracle, all three on the same matrix A."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_fp32_emulation, sart_gpu_semantics

    kw = dict(logarithmic=log, max_iterations=iters, beta_laplace=beta)
    x64, _, _ = sart_gpu_semantics(A, g, L, conv_tolerance=0.0, **kw)
    e32 = max(_rel(sart_fp32_emulation(A, g, L, order=o, **kw)[0], x64) for o in ("blas", "reference"))
    return _rel(x, x64), e32


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("with_lap", [False, True])
def test_solver_on_the_raytraced_matrix(dev, realistic, lap, log, with_lap):
    """The two-pass kernels on exactly widened values: the fp32 two-pass bound of tests/test_gpu_realistic.py, with
    the oracle and the fp32 emulation run on the dequantised matrix."""
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams

    A, G, q = realistic
    L = lap if with_lap else None
    beta = 1e-3
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    np.testing.assert_array_equal(m.to_host(), q.dequantised)
    p = SolverParams(max_iterations=40, conv_tolerance=0.0, beta_laplace=beta)
    s = SARTSolver(m, L, None, p, logarithmic=log, allow_zero_tolerance=True)
    assert not s.use_fused
    np.testing.assert_allclose(s.ray_density64, q.dequantised.astype(np.float64).sum(0), rtol=1e-12)
    np.testing.assert_allclose(s.ray_length64, q.dequantised.astype(np.float64).sum(1), rtol=1e-12)
    for f in (0, 5):
        r = s.solve(G[f])
        assert not r.used_fused and r.iterations == 40
        e, e32 = _errors(r.solution, q.dequantised, G[f], L, log=log, iters=40, beta=beta)
        print(f"f16 two-pass log={log} lap={with_lap} frame {f}: {e:.3e} (fp32 emulation {e32:.3e})")
        assert e <= FACTOR * e32 + SLACK, (f, e, e32)
    assert SARTSolver(m, L, None, p, logarithmic=log, allow_zero_tolerance=True, use_fused=False).use_fused is False
    with pytest.raises(ValueError, match="fused f16 sweep is not built yet"):
        SARTSolver(m, L, None, p, logarithmic=log, allow_zero_tolerance=True, use_fused=True)


def test_engine_refuses_what_it_has_not_built(k, dev):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    m = DenseRTM.synthetic(128, 256, device=dev, storage="f16")
    comm = k.local_comm()

    def cfg(**kw):
        c = k.EngineConfig()
        c.rtm_f16, c.use_fused, c.row_scale = True, False, m.row_scale.data_ptr()
        for name, v in kw.items():
            setattr(c, name, v)
        return c

    args = (0, m.A.data_ptr(), m.npixel, m.nrows_pad, m.nvoxel, m.ld, comm)
    k.Engine(*args, cfg())
    with pytest.raises(ValueError, match="fused f16 sweep is not built yet"):
        k.Engine(*args, cfg(use_fused=True))
    with pytest.raises(ValueError, match="exclusive"):
        k.Engine(*args, cfg(rtm_bf16=True))
    with pytest.raises(ValueError, match="row shards"):
        k.Engine(*args, cfg(column_shard=True))
    with pytest.raises(ValueError, match="needs its row scales"):
        k.Engine(*args, cfg(row_scale=0))
    with pytest.raises(ValueError, match="exclusive"):
        k.MultiFrameEngine(*args, cfg(rtm_bf16=True))


def test_f16_synthetic_problem_and_device_oracle(dev):
    """make_problem(storage="f16") takes g over the stored matrix; the device fp64 oracle dequantises its blocks."""
    from mpi_cuda_sartsolver_amd.models.oracle import sart_oracle_f64
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
    from mpi_cuda_sartsolver_amd.utils.synthetic import make_problem

    prob = make_problem(1000, 2048, seed=3, device=dev, storage="f16", saturate_fraction=0.02)
    assert prob.rtm.is_f16
    g = prob.measurement.cpu().numpy()
    x64 = sart_oracle_f64(prob.rtm, g, 10)
    xh, _, _ = sart_gpu_semantics(prob.rtm.to_host(), g, None, max_iterations=10, conv_tolerance=0.0)
    assert _rel(x64, xh) < 1e-6
    r = SARTSolver(prob.rtm, None, None, SolverParams(max_iterations=10, conv_tolerance=0.0),
                   allow_zero_tolerance=True).solve(g)
    # the shared bound of the solver tests: no further from the fp64 oracle than an fp32 evaluation on the same matrix
    from fp32_bound import check_fp32_bound

    e, e32 = check_fp32_bound(r.solution, prob.rtm.to_host(), g, iterations=10, beta_laplace=0.0)
    print(f"f16 synthetic 1000 x 2048: {e:.3e} (fp32 emulation {e32:.3e})")


# ---------------------------------------------------------------------------------------------- 6. CLI


@pytest.mark.parametrize("extra", [[], ["--batch_frames", "16"]])
def test_cli_rtm_f16(tmp_path, capfd, extra):
    """sartsolver --rtm_f16 frame by frame (two-pass kernels) and with --batch_frames 16 (f16-storage MFMA kernels)
    on HDF5 files of the ray-traced model: every frame against the oracle of the same chain on the emulation's
    dequantised matrix; --profile names the storage, the solver path and the emulation's flushed count."""
    from mpi_cuda_sartsolver_amd import cli
    from mpi_cuda_sartsolver_amd.io.fixtures import make_case

    from test_cli_e2e import chain_errors

    case = make_case(str(tmp_path / "c"), shapes=((32, 32), (32, 32)), grid=(16, 16, 16), raytraced=True,
                     sparse_cameras=("cam_b",), laplacian=True, nframes=4, saturate=0.02, mask_fraction=0.1)
    q = _quantise(case.A)
    out, prof = str(tmp_path / "out.h5"), str(tmp_path / "prof.jsonl")
    batched = "--batch_frames" in extra
    argv = ["--rtm_f16", "-m", "40", "-c", "1e-7", "-l", case.laplacian_file, "-b", "1e-3", "-o", out, "--profile", prof]
    argv += extra + (["--no_guess"] if batched else []) + case.files
    assert cli.main(argv) == 0
    assert capfd.readouterr().out.count("Processed in:") == 4
    e, e32 = chain_errors(case, out, warm=not batched, A=q.dequantised, orders=("blas", "reference"))
    print("cli --rtm_f16", extra, e, e32)
    assert np.all(e <= (MF_FACTOR if batched else FACTOR) * e32 + SLACK), (e, e32)
    load = [json.loads(ln) for ln in open(prof)][0]
    assert load["load"] and load["rtm_storage"] == "f16" and load["f16_flushed"] == q.flushed
    nz = int(np.count_nonzero(case.A))
    assert abs(load["f16_flushed_fraction"] - q.flushed / nz) <= 1e-5 * q.flushed / nz
    assert load["solver_path"] == ("multi-frame f16-storage / f16-storage" if batched else "two-pass")
    assert cli.main(["--rtm_f16", "--rtm_bf16", "-o", out] + case.files) == 1
    assert "exclusive" in capfd.readouterr().err
