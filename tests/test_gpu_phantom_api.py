"""models.phantom.solve_phantoms on the ray-traced 2048 x 512 matrix: three truths (the ring phantom, two isolated
voxels, the dark frame) with 4 replicas each are 15 cold columns of one batch of 16, 40 fixed updates. The columns are
bitwise those of solve_batch on the same frames -- fit_forward of the truths and their perturbed_frames -- and the sums
and scores those of phantom_scores(phantom_sums(...)) on the columns; phantom_sums over 8-column groups against one
column at a time."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NREP, ITERS, SEED = 4, 40, 7
TIMES = [0.5, 1.5, 1.75]


def _solver(dev):
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams
    from mpi_cuda_sartsolver_amd.utils.raytrace import raytraced_rtm

    A, _ = raytraced_rtm(grid=(8, 8, 8))
    return A, MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), None, None,
                                   SolverParams(max_iterations=ITERS, conv_tolerance=0.0, beta_laplace=0.0), batch=16,
                                   allow_zero_tolerance=True)


def test_solve_phantoms_is_solve_batch_on_the_projections():
    from mpi_cuda_sartsolver_amd.models.fit import fit_forward
    from mpi_cuda_sartsolver_amd.models.phantom import SCORE_NAMES, phantom_scores, phantom_sums, solve_phantoms
    from mpi_cuda_sartsolver_amd.models.uncertainty import perturbed_frames
    from mpi_cuda_sartsolver_amd.utils.raytrace import phantom

    dev = torch.device("cuda", 0)
    A, s = _solver(dev)
    truths = np.zeros((3, 512))
    truths[0] = phantom((8, 8, 8), t=0.0)
    truths[1, 77], truths[1, 300] = 1.0, 0.25
    noise = dict(abs=1e-3 * float((A.astype(np.float64) @ truths[0]).max()), shot=0.0, rel=0.02)
    res = solve_phantoms(s, truths, NREP, times=TIMES, seed=SEED, **noise)
    assert len(res) == 3
    F = fit_forward(s.rtm, truths)
    frames = np.concatenate([perturbed_frames(F[k], TIMES[k], NREP, seed=SEED, device=dev, **noise) for k in range(3)])
    cols = s.solve_batch(frames)
    for k, r in enumerate(res):
        assert np.array_equal(r.image, F[k]) and np.array_equal(r.frames, frames[5 * k: 5 * k + 5]) and r.time == TIMES[k]
        assert len(r.columns) == NREP + 1 and r.sums.shape == (NREP + 1, 10)
        X = np.stack([c.solution for c in r.columns])
        for c in range(NREP + 1):
            assert r.columns[c].iterations == ITERS and not r.columns[c].nonfinite
            assert np.array_equal(X[c], cols[5 * k + c].solution), (k, c)
        sums = phantom_sums(X, truths[k], device=dev)
        assert np.array_equal(r.sums, sums)
        assert np.array_equal(sums, np.stack([phantom_sums(X[c], truths[k], device=dev) for c in range(NREP + 1)]))
        want = phantom_scores(sums)
        for name in SCORE_NAMES:
            assert np.array_equal(r.scores[name], want[name], equal_nan=True), (k, name)
    # what the scores say: a cosine is within (0, 1] (Cauchy-Schwarz, up to rounding); the dark truth has no relative
    # error
    assert np.all(res[0].scores["cosine"] > 0.0) and np.all(res[0].scores["cosine"] <= 1.0 + 1e-12)
    assert np.all(np.isnan(res[2].scores["rel_l2"]))
    assert np.all(res[2].sums[1:, 1] > 0.0)  # the clamp's bias on the dark frame: something comes back


def test_phantom_sums_groups_of_eight():
    """More than 8 columns: the groups are separate launches, every column the bits of its own launch."""
    from mpi_cuda_sartsolver_amd.models.phantom import phantom_sums

    rng = np.random.default_rng(1)
    t = rng.random(700)
    t[::3] = 0.0
    X = rng.random((19, 700))
    all_ = phantom_sums(X, t)
    assert all_.shape == (19, 10)
    for c in (0, 7, 8, 15, 16, 18):
        assert np.array_equal(all_[c], phantom_sums(X[c], t))
    with pytest.raises(ValueError):
        phantom_sums(X, t[:-1])
