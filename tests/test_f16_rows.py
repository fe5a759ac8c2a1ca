"""Row-scaled f16 storage of the RTM: the NumPy definition of the format (utils/f16rows.py, the oracle of the device
conversion kernel and of every f16 GPU test) and the quality of the stored matrix on the ray-traced fixture.

Format: H[p, v] = rne_f16(A[p, v] s_p), s_p = 2^clamp(14 - e_p, +-120) for a row maximum m_p = mant 2^e_p with mant in
[0.5, 1) (scaled row maxima in [2^13, 2^14)); s_p = 1 for an all-zero row; f16 subnormals are kept.
"""
import numpy as np
import pytest

from mpi_cuda_sartsolver_amd.utils.f16rows import dequantise_rows_f16, quantise_rows_f16, row_scale_exponents


def _f16(bits):
    return np.ascontiguousarray(bits).view(np.float16).astype(np.float64)


def _mixed_rows(seed=0, n=64, v=300):
    """Rows over 15 decades in random order, entries over a few decades inside a row."""
    rng = np.random.default_rng(seed)
    A = rng.random((n, v), dtype=np.float32) * 10.0 ** rng.uniform(-3, 0, (n, v)).astype(np.float32)
    return (A * rng.permutation(np.logspace(-12, 3, n)).astype(np.float32)[:, None]).astype(np.float32)


def test_scaled_row_maxima_and_exact_inverse():
    A = _mixed_rows()
    q = quantise_rows_f16(A)
    assert q.bits.dtype == np.uint16 and q.scales.dtype == np.float32 and q.dequantised.dtype == np.float32
    scaled_max = np.abs(A.astype(np.float64) * q.scales.astype(np.float64)[:, None]).max(1)
    assert np.all(scaled_max >= 2.0 ** 13) and np.all(scaled_max < 2.0 ** 14)
    inv = np.float32(1) / q.scales
    assert np.all(q.scales * inv == np.float32(1))  # powers of two: scale x inverse == 1 exactly
    assert np.all(np.log2(q.scales.astype(np.float64)) == np.round(np.log2(q.scales.astype(np.float64))))
    # the dequantised matrix is H / s_p exactly, and within half an f16 ulp (2^-11 relative) of A above the
    # subnormal range
    np.testing.assert_array_equal(q.dequantised.astype(np.float64), _f16(q.bits) / q.scales.astype(np.float64)[:, None])
    normal = np.abs(_f16(q.bits)) >= 2.0 ** -14
    rel = np.abs(q.dequantised.astype(np.float64) - A) / np.maximum(np.abs(A), 1e-300)
    assert rel[normal].max() <= 2.0 ** -11
    np.testing.assert_array_equal(dequantise_rows_f16(q.bits, q.scales), q.dequantised)


def test_zero_rows_and_padding():
    A = _mixed_rows(1, 8, 40)
    A[3] = 0
    A[6] = -0.0
    q = quantise_rows_f16(A)
    assert q.scales[3] == 1 and q.scales[6] == 1
    assert not (q.bits[3] & 0x7FFF).any() and not (q.bits[6] & 0x7FFF).any()
    assert not q.dequantised[3].any()


def test_idempotent():
    """Quantising the dequantised matrix reproduces bits and scales. (A row whose maximum rounds UP to a power of
    two in f16 is the one exception in bits, not in value: test_power_of_two_maxima.)"""
    for seed in range(3):
        q = quantise_rows_f16(_mixed_rows(seed))
        top = (q.bits & 0x7FFF).max(1)
        assert np.all(top < 0x7400)  # no stored maximum reached 2^14 on these inputs
        q2 = quantise_rows_f16(q.dequantised)
        np.testing.assert_array_equal(q2.bits, q.bits)
        np.testing.assert_array_equal(q2.scales, q.scales)
        np.testing.assert_array_equal(q2.dequantised, q.dequantised)


@pytest.mark.parametrize("k", [-100, -20, -1, 0, 1, 13, 14, 15, 40, 100])
def test_power_of_two_maxima(k):
    m = np.float32(2.0 ** k)
    below = np.nextafter(m, np.float32(0))
    A = np.zeros((2, 16), dtype=np.float32)
    A[0, :4] = [m, m / 2, -m, m / 3]
    A[1, :4] = [below, below / 2, -below, below / 3]
    q = quantise_rows_f16(A)
    # 2^k = 0.5 x 2^(k + 1): scale 2^(13 - k), stored as 2^13; nextafter(2^k, 0) has exponent k: scale 2^(14 - k),
    # and rounds to nearest even up to 2^14, which f16 holds (the largest stored magnitude of the format)
    assert q.scales[0] == np.float32(2.0 ** (13 - k)) and q.bits[0, 0] == 0x7000 and q.bits[0, 2] == 0xF000
    assert q.scales[1] == np.float32(2.0 ** (14 - k)) and q.bits[1, 0] == 0x7400
    assert q.dequantised[0, 0] == m and q.dequantised[1, 0] == m
    # value-idempotent in both rows (row 1 re-quantises with the scale of row 0: other bits, same values)
    q2 = quantise_rows_f16(q.dequantised)
    np.testing.assert_array_equal(q2.dequantised, q.dequantised)
    assert q2.scales[1] == q.scales[0]


def test_wide_range_inside_a_row():
    """Entries from 1e-30 to 1e3 in one row: 11 bits down to 2^-27 of the maximum, subnormal (absolute error at most
    half of 2^-24 in scaled units) down to 2^-38, zero below."""
    vals = np.array([1e3, 999.0, 1.0, 1e-3, 7e-6, 1e-6, 3e-8, 1e-8, 5e-9, 1e-9, 1e-12, 1e-30, -1e-30, 0.0],
                    dtype=np.float32)
    A = np.stack([vals, vals[::-1]])
    q = quantise_rows_f16(A)
    assert np.all(q.scales == np.float32(2.0 ** 4))  # 1000 = 0.977 x 2^10
    np.testing.assert_array_equal(q.bits[0], q.bits[1][::-1])
    ratio = np.abs(vals.astype(np.float64)) / 1e3
    deq = q.dequantised[0].astype(np.float64)
    normal = ratio >= 2.0 ** -27
    assert np.all(np.abs(deq[normal] - vals[normal]) <= 2.0 ** -11 * np.abs(vals[normal]))
    sub = ~normal
    assert np.all(np.abs(deq[sub] - vals[sub]) <= 2.0 ** -25 / 16.0)
    assert np.all(deq[ratio < 2.0 ** -39] == 0)
    # stored as zero or subnormal: the non-zero entries below 2^-14 in scaled units
    assert quantise_rows_f16(vals[None]).flushed == int(np.count_nonzero(
        (vals != 0) & (np.abs(_f16(q.bits[0])) < 2.0 ** -14)))


def test_non_finite_entries_stay_non_finite():
    A = _mixed_rows(2, 4, 32)
    A[1, 3] = np.nan
    A[1, 7] = np.inf
    A[2, 0] = -np.inf
    q = quantise_rows_f16(A)
    clean = A.copy()
    clean[~np.isfinite(A)] = 0
    np.testing.assert_array_equal(q.scales, quantise_rows_f16(clean).scales)  # the maximum is over finite entries
    assert q.bits[1, 3] == 0x7E00 and q.bits[1, 7] == 0x7C00 and q.bits[2, 0] == 0xFC00
    assert np.isnan(q.dequantised[1, 3]) and np.isposinf(q.dequantised[1, 7]) and np.isneginf(q.dequantised[2, 0])
    fin = np.isfinite(A)
    np.testing.assert_array_equal(q.bits[fin], quantise_rows_f16(clean).bits[fin])


def test_scale_exponent_clamp():
    A = np.zeros((2, 4), dtype=np.float32)
    A[0, 0] = np.float32(2.0 ** -126)  # 14 - (-125) = 139 -> 120
    A[1, 0] = np.float32(1e-45)        # an fp32 subnormal maximum
    assert list(row_scale_exponents(A)) == [120, 120]
    q = quantise_rows_f16(A)
    assert np.all(np.isfinite(q.scales)) and np.all(np.isfinite(np.float32(1) / q.scales))


# ------------------------------------------------------------------------------------------ storage quality


def _round_bf16(A):
    """fp32 values of the bf16 round-to-nearest-even of A (finite inputs)."""
    u = np.ascontiguousarray(A, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def realistic():
    from mpi_cuda_sartsolver_amd.utils.raytrace import phantom, raytraced_rtm

    A, _ = raytraced_rtm(grid=(16, 16, 16))
    rng = np.random.default_rng(3)
    X = np.stack([phantom((16, 16, 16), t=float(t)) for t in (0, 5)])
    G = X @ A.T.astype(np.float64)
    G[rng.random(G.shape) < 0.02] = -1.0  # saturated pixels
    return A, G


def test_storage_quality_on_the_raytraced_matrix(realistic):
    """40 updates of the fp64 oracle on the true matrix, on the row-scaled f16 matrix and on the bf16 matrix (frames
    0 and 5 of the fixture of tests/test_gpu_realistic.py, linear and log): the f16 solution is at most 1/4 as far
    from the true matrix's as the bf16 one (measured 1/8.5 to 1/9.4), and no voxel with ray density above 1e-6
    loses more than 1e-3 of it (measured 3.5e-4)."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics

    A, G = realistic
    Af = quantise_rows_f16(A).dequantised
    Ab = _round_bf16(A)
    for log in (False, True):
        for f in range(2):
            kw = dict(logarithmic=log, max_iterations=40, conv_tolerance=0.0, beta_laplace=0.0)
            x = sart_gpu_semantics(A, G[f], None, **kw)[0]
            xf = sart_gpu_semantics(Af, G[f], None, **kw)[0]
            xb = sart_gpu_semantics(Ab, G[f], None, **kw)[0]
            ef = np.linalg.norm(xf - x) / np.linalg.norm(x)
            eb = np.linalg.norm(xb - x) / np.linalg.norm(x)
            print(f"log={log} frame {(0, 5)[f]}: f16 {ef:.3e} bf16 {eb:.3e} ratio {eb / ef:.2f}")
            assert ef <= 0.25 * eb, (log, f, ef, eb)
    rho = A.astype(np.float64).sum(0)
    rho_f = Af.astype(np.float64).sum(0)
    seen = rho > 1e-6
    loss = np.abs(rho[seen] - rho_f[seen]) / rho[seen]
    print(f"largest ray-density change {loss.max():.3e}")
    assert loss.max() <= 1e-3
    assert np.all(rho_f[seen] > 1e-6)  # no voxel crosses the threshold
