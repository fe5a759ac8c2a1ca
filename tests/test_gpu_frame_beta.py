"""A Laplacian weight per frame in the multi-frame engine (``solve_batch(betas=...)``): every column against the fp64
oracle run at its own weight -- through slots refilled with a frame of another weight, on the fp32 MFMA, split-A and
sparse SpMM paths -- a table of equal entries against the scalar path bit for bit, and the refusal of a warm chain."""
import functools

import numpy as np
import pytest
from fp32_bound import check_fp32_bound

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

P, V = 700, 1000
BETAS = (0.0, 1e-4, 1e-3, 1e-2)
KW = dict(max_iterations=40, conv_tolerance=1e-4)


def _laplacian(dev=None):
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR

    return LaplacianCSR.grid_3d(10, 10, 10, device=dev)


@functools.lru_cache(maxsize=None)
def _problem(nframes, sparse):
    """A (thresholded to ~30 % non-zeros for the sparse shard), frames G with a few saturated pixels."""
    rng = np.random.default_rng(nframes)
    A = rng.random((P, V), dtype=np.float32)
    if sparse:
        A[A < 0.7] = 0.0
    X = rng.random((nframes, V)) + 0.05
    G = X @ A.T.astype(np.float64)
    G[rng.random(G.shape) < 0.03] = -1.0
    return A, G


@functools.lru_cache(maxsize=None)
def _oracle(sparse, log):
    """(status, iterations) of the 5 x 4 columns under the oracle, each at its own weight: computed once per matrix
    and solver kind, shared by the batch widths."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics

    A, G = _problem(5, sparse)
    L = _laplacian()
    out = []
    for k in range(5):
        for b in BETAS:
            _, st, it = sart_gpu_semantics(A, G[k], L, logarithmic=log, beta_laplace=b, **KW)
            out.append((st, it))
    return out


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("path,batch", [("fp32", 16), ("split-a", 32), ("sparse", 16)])
def test_columns_match_the_oracle_at_their_own_weight(log, path, batch):
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM, SparseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    dev = torch.device("cuda", 0)
    sparse = path == "sparse"
    A, G = _problem(5, sparse)
    L = _laplacian(dev)
    rtm = SparseRTM.from_dense(A, device=dev) if sparse else DenseRTM.from_dense(A, device=dev)
    # beta_laplace = 0: without frame_betas the engine would drop the Laplacian
    s = MultiFrameSARTSolver(rtm, L, None, SolverParams(beta_laplace=0.0, **KW), logarithmic=log, batch=batch,
                             frame_betas=True)
    assert s.batch_width == batch
    if not sparse:
        assert s.split_a == (path == "split-a")
    nb = len(BETAS)
    # 20 columns: more than 16 slots, so slots are refilled on the device with a frame of another weight
    res = s.solve_batch(np.repeat(G, nb, axis=0), betas=np.tile(BETAS, 5))
    assert len(res) == 5 * nb
    ref = _oracle(sparse, log)
    for j, r in enumerate(res):
        st, it = ref[j]
        print(f"column {j}: beta {BETAS[j % nb]:g} status {r.status}/{st} iterations {r.iterations}/{it}")
        assert r.status == st
        assert abs(r.iterations - it) <= 2
    for j in (0, (5 * nb) // 2, 5 * nb - 1):
        e, e32 = check_fp32_bound(res[j].solution, A, G[j // nb], L, log=log, iterations=res[j].iterations,
                                  beta_laplace=BETAS[j % nb])
        print(f"column {j}: rel {e:.3e} fp32 emulation {e32:.3e}")
    # the weights matter: a frame's columns differ from each other
    assert not np.array_equal(res[0].solution, res[nb - 1].solution)


@pytest.mark.parametrize("log", [False, True])
def test_equal_table_gives_the_scalar_path_bits(log):
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    dev = torch.device("cuda", 0)
    A, G = _problem(16, False)
    L = _laplacian(dev)
    rtm = DenseRTM.from_dense(A, device=dev)
    scalar = MultiFrameSARTSolver(rtm, L, None, SolverParams(beta_laplace=1e-3, **KW), logarithmic=log, batch=16)
    ref = scalar.solve_batch(G)
    table = MultiFrameSARTSolver(rtm, L, None, SolverParams(beta_laplace=0.0, **KW), logarithmic=log, batch=16,
                                 frame_betas=True)
    res = table.solve_batch(G, betas=[1e-3] * 16)
    for a, b in zip(res, ref):
        assert a.status == b.status and a.iterations == b.iterations
        assert np.array_equal(a.solution, b.solution)
    # and the scalar engine takes a table too (its Laplacian is kept: beta_laplace > 0)
    res2 = scalar.solve_batch(G, betas=[1e-3] * 16)
    for a, b in zip(res2, ref):
        assert a.iterations == b.iterations and np.array_equal(a.solution, b.solution)


def test_chain_with_a_table_is_refused():
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    dev = torch.device("cuda", 0)
    A, G = _problem(5, False)
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), _laplacian(dev), None,
                             SolverParams(beta_laplace=1e-3, **KW), batch=16, frame_betas=True)
    with pytest.raises(ValueError, match="chain"):
        s.solve_batch(G, chain=True, betas=[1e-3] * 5)
    with pytest.raises(ValueError, match="one entry per frame"):
        s.solve_batch(G, betas=[1e-3] * 4)
    # without a Laplacian there is nothing to weigh
    bare = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), None, None, SolverParams(**KW), batch=16)
    with pytest.raises(ValueError, match="Laplacian"):
        bare.solve_batch(G, betas=[1e-3] * 5)
    assert len(s.solve_batch(G, betas=[1e-3] * 5)) == 5  # the engine still runs after the refusals
