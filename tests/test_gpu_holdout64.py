"""The hold-out scoring kernel (csrc/kernels/holdout64.hip) through models.holdout.holdout_sums: bit for bit against
utils.holdout.sums_reference, which adds in the kernel's order (256 lanes over their pixels in order, then the tree), and
against math.fsum within 1e-13 relative -- a sum of n non-negative fp64 terms in any order is within about n 2^-53 of
the exact sum, 2e-13 of it for the 1513 pixels here at most, and the tree keeps the longest chain of additions at
4 + 8 terms. Shapes: cameras of 1, 255, 256, 257 and 1000 pixels (below, at and above one pass of the 256 lanes, several
passes) and a single camera of 300; 1, 5 and 8 columns; image rows longer than the pixels with NaN beyond them; a column
that holds nothing out; a fold absent from a camera; a camera with every pixel excluded; NaN in f, g and ell."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

K = 4
CAMS = (1, 255, 256, 257, 1000)
THR = 1e-6


def _inputs(cams, n, seed, pad=0):
    rng = np.random.default_rng(seed)
    npix = sum(cams)
    g = rng.uniform(0.0, 4.0, npix)
    g[rng.random(npix) < 0.05] = -1.0          # saturated
    g[rng.random(npix) < 0.02] = 0.0           # dark and valid
    ell = rng.uniform(0.5, 2.0, npix)
    ell[rng.random(npix) < 0.05] = 0.0         # no ray: not counted
    fold = rng.integers(0, K, npix).astype(np.int32)
    F = np.full((n, npix + pad), np.nan)
    F[:, :npix] = g[None, :] + rng.normal(0.0, 0.3, (n, npix))
    held = np.resize(np.arange(-1, K, dtype=np.int32), n)
    return F, g, ell, fold, held


def _check(F, g, ell, fold, held, cams, what):
    from mpi_cuda_sartsolver_amd.models.holdout import holdout_sums
    from mpi_cuda_sartsolver_amd.utils.holdout import sums_reference

    got = holdout_sums(F, g, ell, THR, fold, held, cams)
    want = sums_reference(F, g, ell, THR, fold, held, cams)
    assert got.shape == (F.shape[0], len(cams), 6)
    assert np.array_equal(got, want, equal_nan=True), (what, np.argwhere(got != want)[:5])
    return got


def _fsum(F, g, ell, fold, held, cams):
    starts = np.concatenate([[0], np.cumsum(cams)])
    out = np.zeros((F.shape[0], len(cams), 6))
    for j in range(F.shape[0]):
        for m in range(len(cams)):
            H, Kp = [], []
            for p in range(starts[m], starts[m + 1]):
                if g[p] >= 0 and ell[p] > THR:
                    (H if held[j] >= 0 and fold[p] == held[j] else Kp).append(p)
            for q0, S in ((0, H), (3, Kp)):
                out[j, m, q0] = math.fsum((g[p] - F[j, p]) ** 2 for p in S)
                out[j, m, q0 + 1] = math.fsum(g[p] * g[p] for p in S)
                out[j, m, q0 + 2] = len(S)
    return out


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("cams", [CAMS, (300,)], ids=["five-cameras", "one-camera"])
def test_against_the_reference_and_fsum(cams, n):
    F, g, ell, fold, held = _inputs(cams, n, seed=10 * n + len(cams), pad=37)
    got = _check(F, g, ell, fold, held, cams, (cams, n))
    exact = _fsum(F, g, ell, fold, held, cams)
    assert np.array_equal(got[..., [2, 5]], exact[..., [2, 5]])  # the counts are exact
    err = np.abs(got - exact) / np.maximum(np.abs(exact), 1e-300)
    print(f"cams {cams}, n {n}: max relative difference to fsum {err.max():.3e}")
    assert err.max() <= 1e-13
    # the held-out and kept pixels of a column partition the counted pixels of the camera
    starts = np.concatenate([[0], np.cumsum(cams)])
    counted = [(np.nan_to_num(g[a:b], nan=-1) >= 0) & (ell[a:b] > THR) for a, b in zip(starts[:-1], starts[1:])]
    assert np.array_equal(got[..., 2] + got[..., 5], np.tile([c.sum() for c in counted], (n, 1)))
    assert np.all(got[held < 0][..., :3] == 0.0)  # held = -1: nothing is held out


def test_a_value_depends_on_its_column_and_camera_alone():
    from mpi_cuda_sartsolver_amd.models.holdout import holdout_sums

    F, g, ell, fold, held = _inputs(CAMS, 8, seed=3)
    all_ = holdout_sums(F, g, ell, THR, fold, held, CAMS)
    for j in (0, 3, 7):  # one column at a time, in another slot
        assert np.array_equal(holdout_sums(F[j: j + 1], g, ell, THR, fold, held[j: j + 1], CAMS)[0], all_[j])
    # the last camera alone, as the only camera of a frame of its own
    a = sum(CAMS[:-1])
    one = holdout_sums(F[:, a:], g[a:], ell[a:], THR, fold[a:], held, CAMS[-1:])
    assert np.array_equal(one[:, 0], all_[:, -1])


def test_absent_fold_and_excluded_camera():
    F, g, ell, fold, held = _inputs(CAMS, 5, seed=4)
    a, b = 1 + 255, 1 + 255 + 256
    fold[a:b][fold[a:b] == 2] = 3                # fold 2 is absent from camera 2
    c, d = b, b + 257
    g[c:d] = -1.0                                # camera 3: every pixel excluded
    got = _check(F, g, ell, fold, held, CAMS, "absent")
    assert np.all(got[:, 3] == 0.0)              # all six values of every column
    j = int(np.where(held == 2)[0][0])
    assert np.all(got[j, 2, :3] == 0.0) and got[j, 2, 5] > 0


def test_nan_handling():
    cams = (255, 257)
    F, g, ell, fold, held = _inputs(cams, 5, seed=5)
    base = _check(F, g, ell, fold, held, cams, "base")
    assert np.all(np.isfinite(base))
    valid = np.where((g >= 0) & (ell > THR))[0]
    invalid = np.where(g < 0)[0]
    # a NaN f at a pixel that does not count changes nothing
    F2 = F.copy()
    F2[:, invalid[0]] = np.nan
    F2[2, np.where(ell <= THR)[0][0]] = np.nan
    assert np.array_equal(_check(F2, g, ell, fold, held, cams, "nan f, invalid pixel"), base)
    # a NaN f at one counted pixel: exactly that (column, camera) is NaN
    p = int(valid[valid >= 255][3])
    F3 = F.copy()
    F3[1, p] = np.nan
    got = _check(F3, g, ell, fold, held, cams, "nan f, valid pixel")
    nan = np.isnan(got).any(axis=-1)
    want = np.zeros((5, 2), dtype=bool)
    want[1, 1] = True
    assert np.array_equal(nan, want)
    assert np.array_equal(got[~nan], base[~nan])
    # a NaN g or ell makes the pixel one that does not count
    g4, ell4 = g.copy(), ell.copy()
    g4[valid[0]], ell4[valid[1]] = np.nan, np.nan
    got = _check(F, g4, ell4, fold, held, cams, "nan g / ell")
    assert np.all(np.isfinite(got))
    assert np.array_equal((got[..., 2] + got[..., 5]).sum(axis=1), (base[..., 2] + base[..., 5]).sum(axis=1) - 2)


def test_operands_are_checked():
    from mpi_cuda_sartsolver_amd.models.holdout import holdout_sums

    F, g, ell, fold, held = _inputs((300,), 2, seed=6)
    with pytest.raises(ValueError):
        holdout_sums(F[:, :299], g, ell, THR, fold, held, (300,))   # rows shorter than the pixels
    with pytest.raises(ValueError):
        holdout_sums(F, g, ell, THR, fold, held[:1], (300,))
    with pytest.raises(ValueError):
        holdout_sums(F, g[:-1], ell, THR, fold, held, (300,))
    with pytest.raises(ValueError):
        holdout_sums(F, g, ell, THR, fold, held, (200, 50))         # the cameras do not add up to the pixels
