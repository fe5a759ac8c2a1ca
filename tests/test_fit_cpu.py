"""Host side of the fit diagnostics (csrc/native/fit.cpp): cpu_fit_forward on dense fp32 rows and on CSR rows against
NumPy within the fp64 dot-product bound (tests/fit_bound.py), fit_statistics against the NumPy formulas, and hand
cases: every pixel saturated, a camera without a valid pixel, a ray length exactly at the threshold."""
import numpy as np
import pytest

import fit_bound as fb
from mpi_cuda_sartsolver_amd.ops import native


def _dense(P, V, ld, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((P, ld), dtype=np.float32)
    A[:, :V] = rng.random((P, V), dtype=np.float32) * np.exp(rng.normal(0, 3, (P, V))).astype(np.float32)
    A[:, :V][rng.random((P, V)) < 0.3] = 0
    A[:, V:] = np.float32(7.0)  # padding columns must not be read
    return A


@pytest.mark.parametrize("P, V, ld", [(1, 1, 1), (13, 65, 128), (77, 1000, 1000)])
@pytest.mark.parametrize("nv", [1, 3, 8, 11])
def test_cpu_fit_forward_dense(P, V, ld, nv):
    A = _dense(P, V, ld, seed=P + nv)
    rng = np.random.default_rng(1)
    X = np.full((nv, V + 5), np.nan)
    X[:, :V] = rng.normal(size=(nv, V))
    F = native().cpu_fit_forward(A, P, V, X)
    assert F.shape == (nv, P) and F.dtype == np.float64
    F_ref, bound = fb.reference(A[:, :V], X[:, :V])
    fb.assert_image(F, F_ref, bound, f"dense {P}x{V} nv={nv}")
    # a vector's image does not depend on its group
    for j in {0, nv // 2, nv - 1}:
        np.testing.assert_array_equal(native().cpu_fit_forward(A, P, V, X[j:j + 1])[0], F[j])


def _csr(lengths, V, seed):
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for n in lengths] + [[]]).astype(np.int32)
    val = (rng.random(idx.size) + 0.05).astype(np.float32)
    A = np.zeros((len(lengths), V), dtype=np.float32)
    for p, n in enumerate(lengths):
        A[p, idx[ptr[p]:ptr[p + 1]]] = val[ptr[p]:ptr[p + 1]]
    return ptr, idx, val, A


@pytest.mark.parametrize("nv", [1, 5, 8])
def test_cpu_fit_forward_csr(nv):
    lengths = [0, 1, 3, 4, 5, 33, 130, 0, 2]
    V = 200
    ptr, idx, val, A = _csr(lengths, V, seed=3)
    X = np.random.default_rng(2).normal(size=(nv, V))
    F = native().cpu_fit_forward_csr(len(lengths), V, ptr, idx, val, X)
    F_ref, bound = fb.reference(A, X, nterms=np.array(lengths))
    fb.assert_image(F, F_ref, bound, f"csr nv={nv}")
    assert np.all(F[:, 0] == 0) and np.all(F[:, 7] == 0)  # empty rows
    with pytest.raises(ValueError):
        native().cpu_fit_forward_csr(len(lengths), V, ptr, idx + 1000, val, X)


def _stats(f, g, ell, thr, cams):
    return native().fit_statistics(f, g, ell, thr, cams)


def test_fit_statistics_against_numpy():
    rng = np.random.default_rng(5)
    cams = [40, 0, 25, 35]
    P = sum(cams)
    g = rng.random(P) * 10
    g[rng.random(P) < 0.2] = -1.0
    f = g + rng.normal(size=P)
    ell = rng.random(P)
    ell[rng.random(P) < 0.2] = 0.0
    thr = 0.1
    got = _stats(f, g, ell, thr, cams)
    ref = fb.stats_reference(f, g, ell, thr, cams)
    fb.assert_stats(got, ref, np.zeros(P), cams, "random")
    assert got["pixels_camera"][1] == 0 and got["residual_norm_camera"][1] == 0
    assert got["pixels"] == int(((g >= 0) & (ell > thr)).sum())
    # sequential loops: the same numbers whatever the thread count
    n = native()
    before = n.cpu_num_threads()
    try:
        n.cpu_set_num_threads(1)
        one = _stats(f, g, ell, thr, cams)
        n.cpu_set_num_threads(4)
        four = _stats(f, g, ell, thr, cams)
    finally:
        n.cpu_set_num_threads(before)
    for k in fb.FIT_DATASETS[1:]:
        np.testing.assert_array_equal(one[k], four[k])
        np.testing.assert_array_equal(one[k], got[k])


def test_fit_statistics_all_saturated():
    P = 6
    got = _stats(np.ones(P), -np.ones(P), np.ones(P), 1e-6, [2, 4])
    assert got["pixels"] == 0 and got["residual_norm"] == 0 and got["measurement_norm"] == 0
    assert got["residual_max"] == 0
    np.testing.assert_array_equal(got["pixels_camera"], [0, 0])
    np.testing.assert_array_equal(got["residual_norm_camera"], [0, 0])
    np.testing.assert_array_equal(got["measurement_norm_camera"], [0, 0])


def test_fit_statistics_camera_without_valid_pixel():
    g = np.array([1.0, 2.0, -1.0, -1.0, 3.0])
    f = np.array([0.5, 2.0, 9.0, 9.0, 1.0])
    got = _stats(f, g, np.ones(5), 1e-6, [2, 2, 1])
    np.testing.assert_array_equal(got["pixels_camera"], [2, 0, 1])
    np.testing.assert_array_equal(got["residual_norm_camera"], [0.5, 0.0, 2.0])
    np.testing.assert_array_equal(got["measurement_norm_camera"], [np.sqrt(5.0), 0.0, 3.0])
    assert got["residual_norm"] == np.sqrt(0.25 + 4.0) and got["residual_max"] == 2.0 and got["pixels"] == 3


def test_fit_statistics_ray_length_at_threshold_is_excluded():
    thr = 0.125
    g = np.array([1.0, 1.0, 1.0])
    f = np.zeros(3)
    ell = np.array([thr, np.nextafter(thr, 1.0), np.nextafter(thr, 0.0)])
    got = _stats(f, g, ell, thr, [3])
    assert got["pixels"] == 1 and got["residual_norm"] == 1.0 and got["measurement_norm"] == 1.0
    # g = 0 is a valid (dark) pixel, not a saturated one
    got = _stats(np.array([0.5]), np.array([0.0]), np.array([1.0]), thr, [1])
    assert got["pixels"] == 1 and got["residual_norm"] == 0.5 and got["measurement_norm"] == 0.0


def test_fit_statistics_nonfinite_image_shows():
    got = _stats(np.array([np.nan, 1.0]), np.array([1.0, 1.0]), np.ones(2), 0.0, [2])
    assert np.isnan(got["residual_norm"]) and np.isnan(got["residual_max"]) and got["pixels"] == 2


def test_fit_statistics_checks_the_camera_split():
    with pytest.raises(ValueError):
        _stats(np.zeros(3), np.zeros(3), np.ones(3), 0.0, [1, 1])
