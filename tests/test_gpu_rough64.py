"""The fp64 roughness kernel (csrc/kernels/rough64.hip, models/lcurve.py) against NumPy fp64 at the bound of
tests/rough_bound.py: a grid Laplacian whose row count is ragged against the kernel's 32-row tiles and 256-thread
blocks, a random CSR with an empty row, a one-entry row and a row longer than every lane group, 1 / 3 / 8 solutions per
pass, linear and logarithmic (with exact zeros), NaN in the padding of X, and the bits of a wide pass against eight
single ones."""
import functools

import numpy as np
import pytest
import rough_bound

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _laplacian(kind):
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR

    dev = torch.device("cuda", 0)
    if kind == "grid":  # n = 1000: 31 tiles and a quarter, 3 blocks and 232 rows
        return LaplacianCSR.grid_3d(10, 10, 10, device=dev)
    # n = 257: an empty row (0), a one-entry row (1), a 300-entry row with repeated columns (2), the rest 0 .. 12
    rng = np.random.default_rng(7)
    n = 257
    counts = rng.integers(0, 13, n)
    counts[:3] = (0, 1, 300)
    i = np.repeat(np.arange(n), counts)
    j = rng.integers(0, n, i.size)
    v = rng.standard_normal(i.size).astype(np.float32)
    return LaplacianCSR(n, i, j, v, device=dev)


def _solutions(L, nv, log, seed=0):
    """[nv, n + 23]: positive values over eleven decades (log mode: with exact zeros), NaN beyond n."""
    rng = np.random.default_rng(seed + nv)
    X = np.full((nv, L.n + 23), np.nan)
    X[:, : L.n] = 10.0 ** rng.uniform(-8, 3, (nv, L.n))
    if log:
        X[:, : L.n][rng.random((nv, L.n)) < 0.05] = 0.0
    else:
        X[:, : L.n] *= rng.choice([-1.0, 1.0], (nv, L.n))
    return X


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("nv", [1, 3, 8])
@pytest.mark.parametrize("kind", ["grid", "random"])
def test_roughness_matches_numpy(kind, nv, log):
    from mpi_cuda_sartsolver_amd.models.lcurve import roughness, roughness_squared

    L = _laplacian(kind)
    X = _solutions(L, nv, log)
    eta2 = roughness_squared(L, X, log=log)
    ref, bound = rough_bound.reference(L.row_ptr_host, L.col_host, L.val_host, X, log)
    assert eta2.shape == (nv,) and np.all(np.isfinite(eta2)) and np.all(ref > 0)
    for j in range(nv):
        print(f"{kind} nv={nv} log={log} j={j}: eta2 {eta2[j]:.17g} ref {ref[j]:.17g} "
              f"|diff| / bound {abs(eta2[j] - ref[j]) / bound[j]:.3e}")
    assert np.all(np.abs(eta2 - ref) <= bound)
    assert np.array_equal(roughness(L, X, log=log), np.sqrt(eta2))
    # a single vector comes back as a scalar
    assert roughness_squared(L, X[0], log=log) == eta2[0]


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("kind", ["grid", "random"])
def test_wide_pass_equals_single_passes_bitwise(kind, log):
    from mpi_cuda_sartsolver_amd.models.lcurve import roughness_squared

    L = _laplacian(kind)
    X = _solutions(L, 8, log, seed=3)
    wide = roughness_squared(L, X, log=log)
    single = np.array([roughness_squared(L, X[j], log=log) for j in range(8)])
    assert np.array_equal(wide, single)
    # nor does the slot or the group's size matter: 3 + 5, and 11 solutions in two passes
    assert np.array_equal(np.concatenate([roughness_squared(L, X[:3], log=log), roughness_squared(L, X[3:], log=log)]),
                          wide)
    X11 = np.concatenate([X[5:], X])
    assert np.array_equal(roughness_squared(L, X11, log=log), np.concatenate([wide[5:], wide]))
    assert np.array_equal(roughness_squared(L, X, log=log), wide)  # and from run to run


def test_host_laplacian_and_argument_checks():
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.lcurve import roughness_squared

    Ld = _laplacian("grid")
    Lh = LaplacianCSR.grid_3d(10, 10, 10)  # host arrays only: uploaded for the call
    X = _solutions(Ld, 2, False)
    assert np.array_equal(roughness_squared(Lh, X, device=torch.device("cuda", 0)), roughness_squared(Ld, X))
    with pytest.raises(ValueError):
        roughness_squared(Ld, X[:, :999])
    # zero solutions are smooth in linear mode, and constant ones under a graph Laplacian (rows sum to zero)
    assert roughness_squared(Ld, np.zeros(1000)) == 0.0
    assert roughness_squared(Ld, np.full(1000, 3.0)) == 0.0
