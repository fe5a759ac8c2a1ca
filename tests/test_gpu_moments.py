"""The moments kernel (csrc/kernels/moments64.hip) against the NumPy loop in its order: acc += X[r] over the replicas
used, divide, then the squared deviations in the same order. Bounds: c additions and a division move a mean by at most
2 c 2^-53 mean_r |x_r| between two correctly rounded evaluations; a standard deviation follows its mean's error twice
over and adds c + 4 roundings of its own. The kernel is built with contraction off, so the results are expected to be
the loop's bits: the test prints whether they were."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    from mpi_cuda_sartsolver_amd.ops import hip

    return hip()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def reference(X, use):
    """(mean, std, c) by the kernel's statement order, vectorised over the voxels."""
    rows = [r for r in range(X.shape[0]) if use[r]]
    c = len(rows)
    acc = np.zeros(X.shape[1])
    for r in rows:
        acc = acc + X[r]
    mean = acc / c if c > 0 else np.full(X.shape[1], np.nan)
    dev2 = np.zeros(X.shape[1])
    for r in rows:
        e = X[r] - mean
        dev2 = dev2 + e * e
    std = np.sqrt(dev2 / (c - 1)) if c > 1 else np.full(X.shape[1], np.nan)
    return mean, std, c


def _values(n, nvoxel, seed):
    """Voxel scales over 1e-7 .. 1e3, replicas scattered 30 % around them; some voxels constant over the replicas."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-7.0, 3.0, nvoxel)
    X = scale[None, :] * np.abs(1.0 + 0.3 * rng.standard_normal((n, nvoxel)))
    X[:, ::17] = scale[::17]
    return X


def _call(k, dev, X, use, nvoxel, ldx):
    n = X.shape[0]
    Xd = torch.full((n, ldx), float("nan"), dtype=torch.float64, device=dev)
    Xd[:, :nvoxel] = torch.from_numpy(X)
    ud = torch.from_numpy(np.asarray(use, dtype=np.uint8)).to(dev)
    mean = torch.full((ldx,), -7.0, dtype=torch.float64, device=dev)
    std = torch.full((ldx,), -7.0, dtype=torch.float64, device=dev)
    k.moments64(Xd.data_ptr(), ldx, nvoxel, n, ud.data_ptr(), mean.data_ptr(), std.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    assert np.all(mean[nvoxel:] == -7.0) and np.all(std[nvoxel:] == -7.0), "entries beyond nvoxel written"
    return mean[:nvoxel], std[:nvoxel]


def check_moments(mean, std, X, use, what=""):
    """The issue's bounds of mean and std against `reference` on X (shared with tests/test_cli_replicas.py)."""
    ref_m, ref_s, c = reference(X, use)
    if c == 0:
        assert np.all(np.isnan(mean)) and np.all(np.isnan(std))
        return c
    rows = [r for r in range(X.shape[0]) if use[r]]
    em = np.abs(mean - ref_m)
    assert np.all(em <= 2 * c * 2.0 ** -53 * np.mean(np.abs(X[rows]), axis=0)), (what, float(em.max()))
    if c == 1:
        assert np.all(np.isnan(std))
    else:
        es = np.abs(std - ref_s)
        assert np.all(es <= 2 * em + (c + 4) * 2.0 ** -52 * ref_s), (what, float(es.max()))
    same = np.array_equal(mean, ref_m) and np.array_equal(std, ref_s, equal_nan=True)
    print(f"{what} c={c}: bitwise equal to the NumPy loop: {same}")
    return c


def _masks(n):
    full = np.ones(n, dtype=np.uint8)
    drop = full.copy()
    drop[n // 2] = 0
    one = np.zeros(n, dtype=np.uint8)
    one[n - 1] = 1
    return {"all": full, "all but one": drop, "one": one, "none": np.zeros(n, dtype=np.uint8)}


@pytest.mark.parametrize("n", [2, 3, 64])
@pytest.mark.parametrize("nvoxel", [1, 63, 257, 4100])
def test_moments_against_the_numpy_loop(k, dev, nvoxel, n):
    X = _values(n, nvoxel, 100 * n + nvoxel)
    ldx = (nvoxel + 63) // 64 * 64 + 64
    for name, use in _masks(n).items():
        mean, std = _call(k, dev, X, use, nvoxel, ldx)
        c = check_moments(mean, std, X, use, f"nvoxel={nvoxel} n={n} mask '{name}'")
        assert c == {"all": n, "all but one": n - 1, "one": 1, "none": 0}[name]
        if c > 1:  # the statistic it is: against NumPy's own two-pass formulas, loosely
            rows = use.astype(bool)
            varies = np.arange(nvoxel) % 17 != 0
            np.testing.assert_allclose(mean, X[rows].mean(axis=0), rtol=1e-13)
            np.testing.assert_allclose(std[varies], X[rows].std(axis=0, ddof=1)[varies], rtol=1e-9)
            assert np.all(std[~varies] <= 1e-13 * mean[~varies])  # constant voxels: the mean's rounding alone


def test_same_call_twice_gives_identical_bits(k, dev):
    X = _values(64, 4100, 1)
    use = _masks(64)["all but one"]
    a, b = (_call(k, dev, X, use, 4100, 4160) for _ in range(2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_refusals(k, dev):
    x = torch.zeros(128, dtype=torch.float64, device=dev)
    u = torch.ones(2, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="moments64"):
        k.moments64(x.data_ptr(), 63, 64, 2, u.data_ptr(), x.data_ptr(), x.data_ptr(), 0)
    with pytest.raises(RuntimeError, match="moments64"):
        k.moments64(x.data_ptr(), 64, 64, -1, u.data_ptr(), x.data_ptr(), x.data_ptr(), 0)


def test_replica_moments_api(dev):
    from mpi_cuda_sartsolver_amd.models.uncertainty import replica_moments

    X = _values(5, 300, 2)
    mean, std, c = replica_moments(X, use=[1, 1, 0, 1, 1], device=dev)
    assert c == 4
    check_moments(mean, std, X, np.array([1, 1, 0, 1, 1], dtype=np.uint8), "api")
    mean, std, c = replica_moments(X, device=dev)
    assert c == 5
    check_moments(mean, std, X, np.ones(5, dtype=np.uint8), "api, all")
