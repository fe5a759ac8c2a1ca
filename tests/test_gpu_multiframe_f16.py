"""Row-scaled f16 storage in the multi-frame engine (``MfPath`` s16, "f16-storage"): the bf16-storage MFMA kernels
instantiated for f16 tiles (v_mfma_f32_16x16x32_f16, two products per element: A x1 + A x2 with the f16 pieces of
X s_f / (W / s_p) s_f), element by element against fp64 products of the dequantised matrix and the fp32 operands at
the bounds of the f16-pair split-A test (tests/test_gpu_multiframe_bf16.py::test_split_a_backprojection_f16_pairs),
and ``MultiFrameSARTSolver`` on the ray-traced fixture at the multi-frame bound of tests/test_gpu_realistic.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MF_FACTOR, SLACK = 1.03, 2e-8  # tests/test_gpu_realistic.py


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


def _bp_layout(W, nf):
    """[P][nf] in frame order -> the back-projection's slot order [P][16][nf / 16] (mf_bp_slot)."""
    P = W.shape[0]
    return np.ascontiguousarray(W.reshape(P, nf // 16, 16).transpose(0, 2, 1).reshape(P, nf))


def _forward(k, dev, m, X, nf, nsplit, blocked):
    st = _stream(dev)
    Xd = torch.zeros((nf, m.ld), device=dev)
    Xd[:, : X.shape[1]] = torch.from_numpy(X)
    x16 = torch.zeros((2, nf * m.ld), dtype=torch.int16, device=dev)
    xmax = torch.zeros(nf, dtype=torch.int32, device=dev)
    xinv = torch.zeros(nf, device=dev)
    k.mf_split_x16(Xd.data_ptr(), m.ld, nf, x16[0].data_ptr(), x16[1].data_ptr(), xmax.data_ptr(), xinv.data_ptr(), st,
                   False, blocked)
    Fo = torch.zeros((nsplit, m.nrows_pad, nf), device=dev)
    k.mf_forward_s16(m.A.data_ptr(), m.ld, m.npixel, m.nrows_pad, x16[0].data_ptr(), x16[1].data_ptr(), Fo.data_ptr(),
                     nsplit, st, nf, blocked, m.row_scale.data_ptr(), xinv.data_ptr())
    torch.cuda.synchronize()
    return Fo


def _backproject(k, dev, m, W, nf, nsplit, ranges):
    st = _stream(dev)
    Wd = torch.zeros((m.nrows_pad, nf), device=dev)
    Wd[: W.shape[0]] = torch.from_numpy(_bp_layout(W, nf))
    Ws = torch.zeros_like(Wd)
    k.mf_scale_w_rows(Wd.data_ptr(), m.row_scale[m.nrows_pad:].data_ptr(), m.nrows_pad, nf, Ws.data_ptr(), st)
    w16 = torch.zeros((2, nf, m.nrows_pad), dtype=torch.int16, device=dev)
    wmax = torch.zeros(nf, dtype=torch.int32, device=dev)
    inv = torch.zeros(nf, device=dev)
    k.mf_split_w16(Ws.data_ptr(), m.nrows_pad, nf, m.nrows_pad, w16[0].data_ptr(), w16[1].data_ptr(), wmax.data_ptr(),
                   1.0, inv.data_ptr(), st)
    part = torch.zeros((nsplit, m.ld, nf), device=dev)
    for v0, v1 in ranges:
        k.mf_backproject_s16(m.A.data_ptr(), m.ld, m.npixel, w16[0].data_ptr(), w16[1].data_ptr(), m.nrows_pad, nsplit,
                             part.data_ptr(), st, nf, v0, v1, inv.data_ptr())
    torch.cuda.synchronize()
    return part


@pytest.mark.parametrize("nf", [16, 32, 64, 128])
@pytest.mark.parametrize("P,V", [(512, 1024), (1000, 2048), (64, 1024), (2048, 4096), (1000, 1088)])
def test_f16_storage_kernels_per_element(k, dev, P, V, nf):
    """Rows over nine decades (per-row scales), frames over three (per-frame scales). Per frame rel < 1e-6; per
    element within (8 x 2^-22 + 2^-24 sqrt(K)) sum |a| |x| (forward, K = V) / sum |a| |w| (back-projection, K = P):
    the bounds of the f16-pair split-A kernels, which carry a second piece of A that is absent here."""
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    rng = np.random.default_rng(P * 3 + V + nf)
    A = rng.random((P, V), dtype=np.float32)
    A *= np.logspace(-9, 0, P)[rng.permutation(P)].astype(np.float32)[:, None]
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    A64 = _quantise(A).dequantised.astype(np.float64)
    np.testing.assert_array_equal(m.to_host().astype(np.float64), A64)

    X = (rng.random((nf, V)) * np.logspace(-3, 0, nf)[:, None]).astype(np.float32)
    nsf = 3 if m.ld > 1024 else 1
    outs = [_forward(k, dev, m, X, nf, nsf, blk) for blk in (False, True, True)]
    assert torch.equal(outs[0], outs[1]), "blocked and frame-major X planes: the same sums"
    assert torch.equal(outs[1], outs[2]), "two runs must be bitwise equal"
    assert torch.count_nonzero(outs[0][:, P:]) == 0
    F = outs[0].sum(0)[:P].double().cpu().numpy()
    X64 = X.astype(np.float64)
    F_ref = A64 @ X64.T
    for f in range(nf):
        rel = np.linalg.norm(F[:, f] - F_ref[:, f]) / np.linalg.norm(F_ref[:, f])
        assert rel < 1e-6, ("forward", f, rel)
    fscale = np.abs(A64) @ np.abs(X64.T)
    tol = 8 * 2.0 ** -22 + 2.0 ** -24 * np.sqrt(V)
    assert np.all(np.abs(F - F_ref) <= tol * fscale), (np.abs(F - F_ref) / np.maximum(fscale, 1e-300)).max()

    W = ((rng.random((P, nf)) - 0.5) * np.logspace(0, 3, nf)[None, :]).astype(np.float32)
    ns = 3
    vmid = (m.ld // 2) // 128 * 128  # a multiple of every kernel's voxel tile (64 or 128)
    ranges = ((0, vmid), (vmid, m.ld)) if 0 < vmid < m.ld else ((0, m.ld),)
    parts = [_backproject(k, dev, m, W, nf, ns, ranges) for _ in range(2)]
    assert torch.equal(parts[0], parts[1]), "two runs must be bitwise equal"
    B = parts[0].sum(0)[:V].double().cpu().numpy()
    W64 = W.astype(np.float64)
    B_ref = A64.T @ W64
    for f in range(nf):
        rel = np.linalg.norm(B[:, f] - B_ref[:, f]) / np.linalg.norm(B_ref[:, f])
        assert rel < 1e-6, ("back-projection", f, rel)
    bscale = np.abs(A64).T @ np.abs(W64)
    tol = 8 * 2.0 ** -22 + 2.0 ** -24 * np.sqrt(P)
    assert np.all(np.abs(B - B_ref) <= tol * bscale), (np.abs(B - B_ref) / np.maximum(bscale, 1e-300)).max()


@pytest.mark.parametrize("nf", [16, 128])
def test_stored_subnormals_take_part_in_the_products(k, dev, nf):
    """Entries below 2^-27 of their row's maximum are stored as f16 subnormals (kept, not flushed: README). Every
    consumer reads them as stored: the MFMA kernels (f16 subnormal operands are not flushed), the two-pass kernels
    (exact widening) and dequantised(). Exact arithmetic: every product and partial sum below is a small multiple of
    a power of two."""
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    P, V = 64, 1024
    A = np.full((P, V), 2.0 ** -30, dtype=np.float32)
    A[:, 0] = 1.0  # scale 2^13: the other entries are stored as 2^-17, an f16 subnormal (2^7 x 2^-24)
    m = DenseRTM.from_dense(A, device=dev, storage="f16")
    assert m.flushed_count == P * (V - 1)
    np.testing.assert_array_equal(m.to_host(), A)
    X = np.ones((nf, V), dtype=np.float32)
    X[:, 0] = 0.0
    F = _forward(k, dev, m, X, nf, 1, True)[0, :P].cpu().numpy()
    np.testing.assert_array_equal(F, np.full((P, nf), (V - 1) * 2.0 ** -30, dtype=np.float32))
    W = np.ones((P, nf), dtype=np.float32)
    B = _backproject(k, dev, m, W, nf, 1, ((0, m.ld),))[0, :V].cpu().numpy()
    np.testing.assert_array_equal(B[0], np.full(nf, float(P), dtype=np.float32))
    np.testing.assert_array_equal(B[1:], np.full((V - 1, nf), P * 2.0 ** -30, dtype=np.float32))
    # the two-pass forward on the same shard
    xd = torch.zeros(m.ld, device=dev)
    xd[1:V] = 1.0
    f = torch.zeros(m.nrows_pad, device=dev)
    k.forward(0, m.A.data_ptr(), m.ld, P, m.nrows_pad, xd.data_ptr(), 0, 0, f.data_ptr(), 0, 0, 0, _stream(dev), False,
              True, m.row_scale[m.nrows_pad:].data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f[:P].cpu().numpy(), np.full(P, (V - 1) * 2.0 ** -30, dtype=np.float32))


# ---------------------------------------------------------------------------------------------- the solver


@pytest.fixture(scope="module")
def realistic():
    from mpi_cuda_sartsolver_amd.utils.raytrace import phantom, raytraced_rtm

    A, _ = raytraced_rtm(grid=(16, 16, 16))
    rng = np.random.default_rng(3)
    X = np.stack([phantom((16, 16, 16), t=float(t)) for t in range(128)])
    G = X @ A.T.astype(np.float64)
    G[rng.random(G.shape) < 0.02] = -1.0  # saturated pixels (the fixture of tests/test_gpu_realistic.py)
    return A, G, _quantise(A).dequantised


@pytest.fixture(scope="module")
def lap(dev):
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR

    return LaplacianCSR.grid_3d(16, 16, 16, device=dev)


@pytest.fixture(scope="module")
def oracle(realistic, lap):
    """(log, frame) -> (fp64 oracle solution, fp32 emulation's error) on the dequantised matrix: computed once per
    frame and shared by the batch widths."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_fp32_emulation, sart_gpu_semantics

    _, G, Aq = realistic
    cache = {}

    def get(log, f, iters=30, beta=1e-3):
        if (log, f) not in cache:
            kw = dict(logarithmic=log, max_iterations=iters, beta_laplace=beta)
            x64, _, _ = sart_gpu_semantics(Aq, G[f], lap, conv_tolerance=0.0, **kw)
            n = np.linalg.norm(x64)
            e32 = max(np.linalg.norm(sart_fp32_emulation(Aq, G[f], lap, order=o, **kw)[0] - x64) / n
                      for o in ("blas", "reference"))
            cache[(log, f)] = (x64, e32)
        return cache[(log, f)]

    return get


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("batch", [16, 32, 64, 128])
def test_multiframe_solver_on_the_raytraced_matrix(dev, realistic, lap, oracle, batch, log):
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    A, G, _ = realistic
    iters, beta = 30, 1e-3
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev, storage="f16"), lap, None,
                             SolverParams(max_iterations=iters, conv_tolerance=0.0, beta_laplace=beta),
                             logarithmic=log, batch=batch, allow_zero_tolerance=True)
    assert s.batch_width == batch and not s.split_a
    assert s.forward_split == "f16-storage" and s.backproject_split == "f16-storage"
    res = s.solve_batch(G[:batch])
    for f in sorted({0, 1, batch // 2, batch - 1}):
        assert res[f].iterations == iters
        x64, e32 = oracle(log, f)
        e = np.linalg.norm(res[f].solution - x64) / np.linalg.norm(x64)
        print(f"f16-storage batch={batch} log={log} frame {f}: {e:.3e} (fp32 emulation {e32:.3e})")
        assert e <= MF_FACTOR * e32 + SLACK, (f, e, e32)
