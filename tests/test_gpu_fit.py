"""The fit kernels (csrc/kernels/fit64.hip) against F_ref = A_stored.astype(float64) @ x per storage -- fp32, bf16,
row-scaled f16, CSR -- within the fp64 dot-product bound (tests/fit_bound.py), their independence of the grouping
(bitwise), column shards, and ``SARTSolver.fit``. X is allocated [nv][ld] with NaN in the padding and F with NaN in the
rows beyond the shard's, which must come back untouched."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fit_bound as fb
from mpi_cuda_sartsolver_amd.models.fit import fit_forward, fit_forward_device
from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM, SparseRTM
from mpi_cuda_sartsolver_amd.utils.f16rows import quantise_rows_f16

pytestmark = pytest.mark.gpu

# ld above nvoxel; rows no multiple of the workgroup's 16; (130, 2300): more than one 512-column tile per lane and a
# ragged last tile
SHAPES = [(13, 65), (77, 1000), (130, 2300)]
STORAGES = ["fp32", "bf16", "f16"]
NVS = [1, 3, 8]
# an empty row, every remainder of the 4-entry unroll, rows longer than 4 L (L = 4 and 32)
SPARSE_LENGTHS = [0, 1, 3, 4, 5, 33, 130, 2, 0, 7]
SPARSE_V = 300


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _dense(P, V, storage):
    """(A_stored fp32 [P, V], device shard) of one shape and storage"""
    rng = np.random.default_rng(100 * P + V)
    if storage == "f16":
        # entries spanning 1e-9 .. 1 within every row (stored subnormals, scales != 1) and one all-zero row
        A = (10.0 ** rng.uniform(-9, 0, (P, V))).astype(np.float32)
        A[:, 0] = 1.0
        A *= (2.0 ** rng.integers(-6, 7, (P, 1))).astype(np.float32)
        A[P // 2] = 0
        q = quantise_rows_f16(A)
        stored = np.asarray(q[2], dtype=np.float32)
        assert q[3] > 0 and np.any(np.asarray(q[1])[:P] != 1)
    else:
        A = rng.random((P, V), dtype=np.float32)
        A[rng.random((P, V)) < 0.2] = 0
        stored = fb.round_bf16(A) if storage == "bf16" else A
    m = DenseRTM.from_dense(A, device=_dev(), storage=storage)
    assert m.ld % 64 == 0 and m.ld > V
    np.testing.assert_array_equal(m.to_host(), stored)  # the reference's matrix is the shard's
    return stored, m


@functools.lru_cache(maxsize=None)
def _sparse():
    rng = np.random.default_rng(9)
    ptr = np.concatenate([[0], np.cumsum(SPARSE_LENGTHS)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(SPARSE_V, size=n, replace=False)) for n in SPARSE_LENGTHS]).astype(np.int32)
    val = ((rng.random(idx.size) + 0.05) * 10.0 ** rng.uniform(-4, 2, idx.size)).astype(np.float32)
    A = np.zeros((len(SPARSE_LENGTHS), SPARSE_V), dtype=np.float32)
    for p in range(len(SPARSE_LENGTHS)):
        A[p, idx[ptr[p]:ptr[p + 1]]] = val[ptr[p]:ptr[p + 1]]
    m = SparseRTM(len(SPARSE_LENGTHS), SPARSE_V, ptr, idx, val, device=_dev())
    assert m.ld > SPARSE_V
    return A, m


@functools.lru_cache(maxsize=None)
def _x(V, nv=8):
    return np.random.default_rng(V).normal(size=(nv, V)) * 10.0 ** np.random.default_rng(V + 1).uniform(-3, 3, (nv, 1))


def _run(m, X, lanes=0):
    """One pass with NaN in X's padding and in F; returns F [nv, P] after checking the untouched rows."""
    nv, V = X.shape
    dev = m.device
    Xd = torch.full((nv, m.ld), float("nan"), dtype=torch.float64, device=dev)
    Xd[:, :V] = torch.from_numpy(X)
    Fd = torch.full((nv, m.nrows_pad), float("nan"), dtype=torch.float64, device=dev)
    Xt = torch.full((m.ld, 8), float("nan"), dtype=torch.float64, device=dev) if hasattr(m, "nnz") else None
    fit_forward_device(m, Xd, nv, Fd, Xt=Xt, lanes=lanes, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    F = Fd.cpu().numpy()
    assert np.all(np.isnan(F[:, m.npixel:])), "rows beyond the shard's were written"
    return F[:, : m.npixel]


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("P, V", SHAPES)
@pytest.mark.parametrize("storage", STORAGES)
def test_fit_dense_against_reference(storage, P, V, nv):
    stored, m = _dense(P, V, storage)
    X = _x(V)[:nv]
    F = _run(m, X)
    F_ref, bound = fb.reference(stored, X)
    fb.assert_image(F, F_ref, bound, f"{storage} {P}x{V} nv={nv}")
    if storage == "f16":
        assert np.all(F[:, P // 2] == 0)  # the all-zero row


@pytest.mark.parametrize("lanes", [4, 32])
@pytest.mark.parametrize("nv", NVS)
def test_fit_sparse_against_reference(nv, lanes):
    A, m = _sparse()
    X = _x(SPARSE_V)[:nv]
    F = _run(m, X, lanes)
    F_ref, bound = fb.reference(A, X, nterms=np.array(SPARSE_LENGTHS))
    fb.assert_image(F, F_ref, bound, f"csr nv={nv} lanes={lanes}")
    assert np.all(F[:, [0, 8]] == 0)  # empty rows


@pytest.mark.parametrize("storage", STORAGES + ["sparse"])
def test_fit_grouping_independence(storage):
    """F[j] of an nv = 8 pass (and of an nv = 3 pass) is the nv = 1 pass on vector j, bit for bit"""
    if storage == "sparse":
        _, m = _sparse()
        V = SPARSE_V
    else:
        P, V = SHAPES[2]
        _, m = _dense(P, V, storage)
    X = _x(V)
    F8 = _run(m, X)
    for j in (0, 3, 7):  # the first, a middle and the last slot
        np.testing.assert_array_equal(_run(m, X[j:j + 1])[0], F8[j], err_msg=f"{storage} slot {j} of 8")
    F3 = _run(m, X[4:7])
    for j in range(3):
        np.testing.assert_array_equal(F3[j], F8[4 + j], err_msg=f"{storage} slot {j} of 3")
    # and of the grid: fit_forward's groups of a longer list
    F11 = fit_forward(m, np.concatenate([X[5:], X]))
    np.testing.assert_array_equal(F11[3:], F8)
    np.testing.assert_array_equal(F11[:3], F8[5:])


def test_fit_refuses_shapes_without_a_kernel():
    _, m = _dense(*SHAPES[0], "fp32")
    dev = m.device
    Xd = torch.zeros((9, m.ld), dtype=torch.float64, device=dev)
    Fd = torch.zeros((9, m.nrows_pad), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="fit64: no kernel for nv = 9"):
        fit_forward_device(m, Xd, 9, Fd)
    _, s = _sparse()
    Xs = torch.zeros((1, s.ld), dtype=torch.float64, device=dev)
    Fs = torch.zeros((1, s.nrows_pad), dtype=torch.float64, device=dev)
    Xt = torch.zeros((s.ld, 8), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="fit64_csr: no kernel for 5 lanes"):
        fit_forward_device(s, Xs, 1, Fs, Xt=Xt, lanes=5)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_fit_column_shards_sum_to_the_full_image(storage):
    P, V = SHAPES[1]
    stored, _ = _dense(P, V, storage)
    A = _dense(P, V, "fp32")[0]  # the fp32 source of both storages
    X = _x(V)[:3]
    V1 = 437
    parts = []
    for c0, c1 in ((0, V1), (V1, V)):
        m = DenseRTM.from_dense(np.ascontiguousarray(A[:, c0:c1]), device=_dev(), col_offset=c0, nvoxel_total=V,
                                storage=storage)
        assert m.is_column_shard
        parts.append(fit_forward(m, np.ascontiguousarray(X[:, c0:c1])))
    F_ref, bound = fb.reference(stored, X)
    fb.assert_image(parts[0] + parts[1], F_ref, bound, f"{storage} column shards")


@pytest.mark.parametrize("kind", ["fp32", "sparse"])
def test_solver_fit(kind):
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams

    rng = np.random.default_rng(4)
    if kind == "sparse":
        A, m = _sparse()
        nterms = np.array(SPARSE_LENGTHS)
    else:
        A, m = _dense(*SHAPES[1], "fp32")
        nterms = None
    P, V = A.shape
    g = A.astype(np.float64) @ (rng.random(V) + 0.1)
    g[rng.random(P) < 0.1] = -1.0  # saturated pixels
    cams = [P // 3, P - P // 3]
    s = SARTSolver(m, None, None, SolverParams(max_iterations=5, conv_tolerance=1e-9))
    x = s.solve(g).solution
    res = s.fit(g, x, camera_pixels=cams)
    F_ref, bound = fb.reference(A, x, nterms)
    fb.assert_image(res.image[None, :], F_ref, bound, f"SARTSolver.fit {kind}")
    ell = A.astype(np.float64).sum(axis=1)
    ref = fb.stats_reference(F_ref[0], g, ell, s.params.ray_length_threshold, cams)
    got = dict(residual_norm=res.residual_norm, measurement_norm=res.measurement_norm, residual_max=res.residual_max,
               pixels=res.pixels, residual_norm_camera=res.residual_norm_camera,
               measurement_norm_camera=res.measurement_norm_camera, pixels_camera=res.pixels_camera)
    fb.assert_stats(got, ref, bound[0], cams, f"SARTSolver.fit {kind}")
    assert 0 < res.pixels < P and np.isfinite(res.relative_residual)
