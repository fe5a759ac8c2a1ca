"""models.holdout.solve_holdout on the ray-traced 2048 x 4096 matrix of tests/test_gpu_realistic.py, its pixels split as
two cameras of 1024, K = 3 pixel folds and a ladder of three Laplacian weights: 12 cold columns of one batch of 16, 20
fixed updates. Every column is held against the fp64 oracle on the NumPy-masked frame for its recorded update count at
the beta-scan column rule (the fp32 emulation's error), the sums against the kernel on the fp64 projections of the
returned columns, the scores against the native function on the returned sums, and the selection against their argmin."""
import numpy as np
import pytest

from fp32_bound import fp32_errors

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

K, ITERS, SEED = 3, 20, 0
BETAS = [0.0, 1e-3, 1e-2]
CAMS = (1024, 1024)
FACTOR, SLACK = 1.0, 1e-6  # the beta-scan column rule (tests/test_cli_beta_scan.py)


@pytest.fixture(scope="module")
def solved():
    from mpi_cuda_sartsolver_amd.models.holdout import solve_holdout
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams
    from mpi_cuda_sartsolver_amd.utils.holdout import folds
    from mpi_cuda_sartsolver_amd.utils.raytrace import phantom, raytraced_rtm

    dev = torch.device("cuda", 0)
    A, _ = raytraced_rtm(grid=(16, 16, 16))
    g = A.astype(np.float64) @ phantom((16, 16, 16), t=0.0)
    g[np.random.default_rng(3).random(g.size) < 0.02] = -1.0  # saturated pixels
    L = LaplacianCSR.grid_3d(16, 16, 16, device=dev)
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), L, None,
                             SolverParams(max_iterations=ITERS, conv_tolerance=0.0, beta_laplace=2e-3), batch=16,
                             allow_zero_tolerance=True, frame_betas=True)
    f = folds(g.size, K, SEED)
    return A, g, L, f, s, solve_holdout(s, g, f, K, betas=BETAS, camera_pixels=CAMS)


def test_columns_against_the_oracle_on_the_masked_frames(solved):
    from mpi_cuda_sartsolver_amd.utils.holdout import masked_frames

    A, g, L, f, _, r = solved
    M = masked_frames(g, f, K)
    assert np.array_equal(r.frames, M) and np.array_equal(r.folds, f) and list(r.betas) == BETAS
    assert len(r.columns) == len(BETAS) and all(len(c) == K + 1 for c in r.columns)
    for i, beta in enumerate(BETAS):
        for c in range(K + 1):
            col = r.columns[i][c]
            assert col.iterations == ITERS and not col.nonfinite
            e, e32 = fp32_errors(col.solution, A, M[c], L, iterations=col.iterations, beta_laplace=beta)
            print(f"beta {beta:g} column {c}: {col.iterations} updates, rel {e:.3e} fp32 emulation {e32:.3e}")
            assert e <= FACTOR * e32 + SLACK, (i, c, e, e32)


def test_sums_scores_and_selection(solved):
    from mpi_cuda_sartsolver_amd.models.fit import fit_forward
    from mpi_cuda_sartsolver_amd.models.holdout import holdout_scores, holdout_sums
    from mpi_cuda_sartsolver_amd.ops import native
    from mpi_cuda_sartsolver_amd.utils.holdout import scores

    A, g, _, f, s, r = solved
    nb, nc = len(BETAS), K + 1
    assert r.sums.shape == (nb, nc, 2, 6)
    X = np.stack([c.solution for cols in r.columns for c in cols])
    ell = fit_forward(s.rtm, np.ones(s.rtm.nvoxel))
    held = np.tile(np.arange(-1, K, dtype=np.int32), nb)
    again = holdout_sums(fit_forward(s.rtm, X), g, ell, s.params.ray_length_threshold, f, held, CAMS)
    assert np.array_equal(r.sums.reshape(nb * nc, 2, 6), again)
    # every counted pixel is held out exactly once over the K masked columns, whatever the weight
    counted = int(((g >= 0) & (ell > s.params.ray_length_threshold)).sum())
    assert np.all(r.sums[:, 1:, :, 2].sum(axis=(1, 2)) == counted) and np.all(r.sums[:, 0, :, 5].sum(axis=1) == counted)
    fallback = int(native().holdout_fallback(np.array(BETAS), 2e-3))
    assert fallback == 1
    want = holdout_scores(r.sums, np.ones((nb, nc)), fallback)
    ref = scores(r.sums, np.ones((nb, nc)), fallback)
    for name in ("cv_error", "cv_relative", "train_error", "cv_error_camera", "eligible"):
        assert np.array_equal(getattr(r.scores, name), getattr(want, name)), name
        assert np.array_equal(getattr(r.scores, name), ref[name]), name
    print("cv_error", r.scores.cv_error, "train_error", r.scores.train_error, "selected", r.scores.selected)
    assert np.all(r.scores.eligible == 1) and r.scores.found
    assert r.scores.selected == int(np.argmin(r.scores.cv_error)) == want.selected
    assert r.result is r.columns[r.scores.selected][0]


def test_without_a_ladder_and_the_exports(solved):
    from mpi_cuda_sartsolver_amd import models
    from mpi_cuda_sartsolver_amd.models import holdout
    from mpi_cuda_sartsolver_amd.utils.holdout import folds

    assert models.solve_holdout is holdout.solve_holdout and models.holdout_sums is holdout.holdout_sums
    _, g, _, _, s, r = solved
    cam = folds(g.size, camera_pixels=CAMS)
    one = holdout.solve_holdout(s, g, cam, 2, camera_pixels=CAMS)  # leave one camera out, at the solver's own weight
    assert list(one.betas) == [2e-3] and one.sums.shape == (1, 3, 2, 6) and one.scores.selected == 0
    # camera m is held out by column m + 1 alone
    assert np.all(one.sums[0, 1, 1, :3] == 0) and np.all(one.sums[0, 2, 0, :3] == 0)
    assert one.scores.cv_error_camera[0, 0] == np.sqrt(one.sums[0, 1, 0, 0] / one.sums[0, 1, 0, 2])
    assert one.scores.cv_error_camera[0, 1] == np.sqrt(one.sums[0, 2, 1, 0] / one.sums[0, 2, 1, 2])
    with pytest.raises(ValueError):
        holdout.solve_holdout(s, g, cam, 1, camera_pixels=CAMS)
