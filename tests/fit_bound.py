"""References and error bounds shared by the fit tests (tests/test_*fit*.py).

An fp64 dot of n terms, fused or not and in any order, is within gamma_n sum |a_v x_v| of the exact value
(gamma_n ~ n 2^-53), and NumPy's reference carries the same bound, so per pixel

    |F - F_ref| <= 2 (n + 2) 2^-53 (|A_stored| |x|)_p

with n the row's term count (nvoxel for dense shards, the row's entries for sparse ones) and A_stored the matrix as
stored (widening fp32 / bf16 / f16 to fp64 is exact). The residual norm follows by the triangle inequality,
|r - r_ref| <= ||bound||_2 + 4 P 2^-53 r_ref, the measurement norm to 4 P 2^-53 relative, the pixel counts exactly, the
residual maximum within the largest per-pixel bound. Reference statistics always come from F_ref.
"""
import numpy as np

U = 2.0 ** -53


def round_bf16(A):
    """fp32 values of the bf16 round-to-nearest-even rounding of an fp32 array (finite values)."""
    u = np.ascontiguousarray(A, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(A))


def reference(A_stored, X, nterms=None):
    """F_ref [nv, P] = X A_stored^T in fp64 and the per-pixel bound [nv, P]. nterms: terms per row (default: the
    number of columns)."""
    A = np.asarray(A_stored, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n = np.full(A.shape[0], A.shape[1]) if nterms is None else np.asarray(nterms)
    F = X @ A.T
    bound = 2.0 * (n[None, :] + 2) * U * (np.abs(X) @ np.abs(A).T)
    return F, bound


def assert_image(F, F_ref, bound, what=""):
    err = np.abs(np.asarray(F) - F_ref)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: max |F - F_ref| / bound = {worst:.3e}")
    assert np.all(np.isfinite(np.asarray(F))), what
    assert np.all(err <= bound), f"{what}: {worst:.3e} of the bound"


def stats_reference(f_ref, g, ell, threshold, camera_pixels):
    """The statistics of docs/FORMATS.md from a reference image, in NumPy."""
    S = (g >= 0) & (ell > threshold)
    r = np.where(S, g - f_ref, 0.0)
    gg = np.where(S, g, 0.0)
    edges = np.concatenate([[0], np.cumsum(camera_pixels)])
    return dict(S=S, residual_norm=np.sqrt(np.sum(r * r)), measurement_norm=np.sqrt(np.sum(gg * gg)),
                residual_max=float(np.max(np.abs(r))) if S.any() else 0.0, pixels=int(S.sum()),
                residual_norm_camera=np.array([np.sqrt(np.sum(r[a:b] ** 2)) for a, b in zip(edges[:-1], edges[1:])]),
                measurement_norm_camera=np.array([np.sqrt(np.sum(gg[a:b] ** 2)) for a, b in zip(edges[:-1], edges[1:])]),
                pixels_camera=np.array([int(S[a:b].sum()) for a, b in zip(edges[:-1], edges[1:])]))


def assert_stats(got, ref, bound, camera_pixels, what=""):
    """got: mapping with the /fit statistics of one frame; ref: stats_reference of F_ref; bound: the per-pixel bound."""
    P = bound.size
    S = ref["S"]
    b = np.where(S, bound, 0.0)
    edges = np.concatenate([[0], np.cumsum(camera_pixels)])
    assert int(got["pixels"]) == ref["pixels"], what
    np.testing.assert_array_equal(np.asarray(got["pixels_camera"]).astype(np.int64), ref["pixels_camera"])
    tol_r = np.linalg.norm(b) + 4 * P * U * ref["residual_norm"]
    print(f"{what}: residual_norm {float(got['residual_norm']):.17g} ref {ref['residual_norm']:.17g} tol {tol_r:.3e}")
    assert abs(float(got["residual_norm"]) - ref["residual_norm"]) <= tol_r, what
    assert abs(float(got["measurement_norm"]) - ref["measurement_norm"]) <= 4 * P * U * ref["measurement_norm"], what
    assert abs(float(got["residual_max"]) - ref["residual_max"]) <= (b.max() if P else 0.0), what
    for c, (a0, a1) in enumerate(zip(edges[:-1], edges[1:])):
        tol = np.linalg.norm(b[a0:a1]) + 4 * P * U * ref["residual_norm_camera"][c]
        assert abs(float(got["residual_norm_camera"][c]) - ref["residual_norm_camera"][c]) <= tol, (what, c)
        assert abs(float(got["measurement_norm_camera"][c]) - ref["measurement_norm_camera"][c]) <= \
            4 * P * U * ref["measurement_norm_camera"][c], (what, c)


FIT_DATASETS = ("image", "residual_norm", "measurement_norm", "residual_max", "pixels", "residual_norm_camera",
                "measurement_norm_camera", "pixels_camera")


def read_fit(native, path):
    """Every /fit dataset and /solution/value, /solution/time of an output file (float64 arrays with their shapes)."""
    d = {k: native.read_dataset_f64(path, "fit/" + k) for k in FIT_DATASETS}
    d["value"] = native.read_dataset_f64(path, "solution/value")
    d["time"] = native.read_dataset_f64(path, "solution/time")
    return d


def check_fit_file(native, path, A_stored, frames, camera_pixels, threshold=1e-6, nterms=None, what=""):
    """Every row of the /fit group of `path` against A_stored @ value[k] (value read from the same file) and the
    statistics in NumPy. frames: the measured composite frame of every stored row."""
    d = read_fit(native, path)
    T = d["time"].size
    assert d["value"].shape[0] == T and len(frames) == T
    assert d["image"].shape == (T, A_stored.shape[0]), d["image"].shape
    assert d["residual_norm_camera"].shape == (T, len(camera_pixels))
    ell = np.asarray(A_stored, dtype=np.float64).sum(axis=1)
    F_ref, bound = reference(A_stored, d["value"], nterms)
    assert_image(d["image"], F_ref, bound, what)
    for k in range(T):
        ref = stats_reference(F_ref[k], np.asarray(frames[k], dtype=np.float64), ell, threshold, camera_pixels)
        assert_stats({n: d[n][k] for n in FIT_DATASETS[1:]}, ref, bound[k], camera_pixels, f"{what} frame {k}")
    return d
