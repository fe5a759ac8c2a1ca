"""models.uncertainty.solve_replicas on the ray-traced 2048 x 512 matrix: 15 replicas and the nominal frame as the 16
cold columns of one batch, 40 fixed updates. Every column within the fp32 bound of the fp64 oracle on the frame the
NumPy emulation gives (FACTOR and SLACK of tests/test_gpu_realistic.py: a batch of 16 runs the fp32 MFMA path), and the
moments no further from the oracle's than the columns are: with D the replica solutions minus their oracles, centring
is a projection, so ||d std||_2 <= sqrt(sum_r ||D_r||_2^2 / (N - 1)) and ||d mean||_2 <= max_r ||D_r||_2."""
import numpy as np
import pytest

from fp32_bound import ORDERS, rel

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FACTOR, SLACK = 1.0, 2e-8  # tests/test_gpu_realistic.py
NREP, ITERS, TIME, SEED = 15, 40, 0.125, 42
NOISE = dict(shot=0.0, rel=0.02)  # with abs at 1e-3 of the frame's maximum


def test_solve_replicas_on_the_raytraced_matrix():
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.reference import sart_fp32_emulation, sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams
    from mpi_cuda_sartsolver_amd.models.uncertainty import solve_replicas
    from mpi_cuda_sartsolver_amd.utils import philox
    from mpi_cuda_sartsolver_amd.utils.raytrace import phantom, raytraced_rtm

    dev = torch.device("cuda", 0)
    A, _ = raytraced_rtm(grid=(8, 8, 8))
    assert A.shape == (2048, 512)
    g = phantom((8, 8, 8), t=0.0) @ A.T.astype(np.float64)
    g[np.random.default_rng(3).random(g.size) < 0.02] = -1.0  # saturated pixels
    noise = dict(abs=1e-3 * float(g.max()), **NOISE)
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), None, None,
                             SolverParams(max_iterations=ITERS, conv_tolerance=0.0, beta_laplace=0.0), batch=16,
                             allow_zero_tolerance=True)
    res = solve_replicas(s, g, TIME, NREP, seed=SEED, **noise)
    ref = philox.perturb(g, TIME, NREP, noise["abs"], noise["shot"], noise["rel"], SEED)
    np.testing.assert_allclose(res.frames, ref, rtol=0, atol=1e-12 * (np.abs(g).max() + 1.0))
    assert res.count == NREP and len(res.replicas) == NREP
    cols = [res.nominal, *res.replicas]
    X64 = []
    for r, col in enumerate(cols):
        assert col.iterations == ITERS and not col.nonfinite
        # fp32_bound.fp32_errors, keeping the oracle's solution for the moments below
        kw = dict(logarithmic=False, max_iterations=ITERS, beta_laplace=0.0, x_prev=None)
        x64 = sart_gpu_semantics(A, ref[r], None, conv_tolerance=0.0, **kw)[0]
        e32 = max(rel(sart_fp32_emulation(A, ref[r], None, order=o, **kw)[0], x64) for o in ORDERS)
        e = rel(col.solution, x64)
        print(f"replica {r}: rel {e:.3e} fp32 emulation {e32:.3e}")
        assert e <= FACTOR * e32 + SLACK, (r, e, e32)
        X64.append(x64)
    X64 = np.stack(X64[1:])
    D = np.stack([c.solution for c in res.replicas]) - X64
    norms = np.linalg.norm(D, axis=1)
    d_std = np.linalg.norm(res.std - X64.std(axis=0, ddof=1))
    d_mean = np.linalg.norm(res.mean - X64.mean(axis=0))
    print(f"||d std|| {d_std:.3e} bound {np.sqrt((norms ** 2).sum() / (NREP - 1)):.3e}; ||d mean|| {d_mean:.3e} bound "
          f"{norms.max():.3e}; ||std|| / ||x0|| {np.linalg.norm(res.std) / np.linalg.norm(res.nominal.solution):.3e}")
    assert d_std <= np.sqrt((norms ** 2).sum() / (NREP - 1))
    assert d_mean <= norms.max()
