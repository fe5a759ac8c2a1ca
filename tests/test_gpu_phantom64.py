"""The phantom scoring kernel alone (csrc/kernels/phantom64.hip): ten fp64 values per column against a truth.

Sums: against math.fsum of the fp64 terms (the terms as NumPy rounds them: a product is one rounding, (x - t)^2 two),
within (nvoxel + 4) 2^-53 sum|term| -- any order of fp64 additions of nvoxel terms stays within (nvoxel - 1) u sum|term|
to first order, u = 2^-53, and the margin covers the second-order part at these sizes. Maxima: exact. A column's ten
values are bitwise the same for nv = 1 .. 8 and in every slot; NaN in the padding of X and t (ldx > nvoxel) changes
nothing. Sizes: one voxel, around a wave (63, 64, 65), several tiles with a ragged end (2049), and 70 001, which needs
several workgroups and the second stage's strided partials."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 2049, 70001]
NAMES = ("s_t", "s_x", "s_tt", "s_xx", "s_xt", "s_dd", "s_in", "m_d", "m_t", "m_x")


def _launch(X, t, nvoxel, nv, ldx=None):
    """sums [nv, 10] of the first nv rows of the device tensor X [>= nv, ldx] against t."""
    from mpi_cuda_sartsolver_amd.ops import hip

    k = hip()
    dev = X.device
    sums = torch.full((8, 10), float("nan"), dtype=torch.float64, device=dev)
    scratch = torch.full((int(k.phantom64_scratch_elems(nvoxel)),), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        k.phantom64(X.data_ptr(), int(ldx if ldx is not None else X.shape[1]), nvoxel, nv, t.data_ptr(), sums.data_ptr(),
                    scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        out = sums.cpu().numpy()
    assert np.all(np.isnan(out[nv:])), "slots beyond nv are not written"
    return out[:nv]


def _terms(x, t):
    d = x - t
    return [t, x, t * t, x * x, x * t, d * d, np.where(t > 0, x, 0.0)]


def check_sums(got, x, t, what):
    """got [10] against fsum of the terms and the exact maxima."""
    n = x.size
    for q, term in enumerate(_terms(x, t)):
        want, scale = math.fsum(term), math.fsum(np.abs(term))
        bound = (n + 4) * 2.0 ** -53 * scale
        err = abs(float(got[q]) - want)
        print(f"{what} {NAMES[q]}: |err| {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, NAMES[q], got[q], want, bound)
    assert got[7] == np.abs(x - t).max() and got[8] == t.max() and got[9] == x.max(), (what, got[7:])


def _data(nvoxel, nc=8, seed=0):
    rng = np.random.default_rng(seed + nvoxel)
    t = rng.random(nvoxel) * 10.0 ** rng.integers(-3, 4, size=nvoxel)
    t[rng.random(nvoxel) < 0.3] = 0.0
    X = np.abs(t[None, :] * (1.0 + 0.3 * rng.standard_normal((nc, nvoxel))) + 0.05 * rng.random((nc, nvoxel)))
    X[:, rng.random(nvoxel) < 0.1] = 0.0
    return X, t


@pytest.mark.parametrize("nvoxel", SIZES)
def test_sums_and_maxima(nvoxel):
    dev = torch.device("cuda", 0)
    X, t = _data(nvoxel)
    got = _launch(torch.from_numpy(X).to(dev), torch.from_numpy(t).to(dev), nvoxel, 8)
    assert np.all(np.isfinite(got))
    for j in range(8):
        check_sums(got[j], X[j], t, f"nvoxel {nvoxel} column {j}")


@pytest.mark.parametrize("nvoxel", SIZES)
def test_a_column_does_not_depend_on_nv_the_slot_or_the_padding(nvoxel):
    dev = torch.device("cuda", 0)
    X, t = _data(nvoxel, seed=1)
    ref = _launch(torch.from_numpy(X).to(dev), torch.from_numpy(t).to(dev), nvoxel, 8)
    # ldx > nvoxel, NaN in the padding of both operands
    ldx = (nvoxel + 63) // 64 * 64 + 64
    Xp = torch.full((8, ldx), float("nan"), dtype=torch.float64, device=dev)
    tp = torch.full((ldx,), float("nan"), dtype=torch.float64, device=dev)
    Xp[:, :nvoxel] = torch.from_numpy(X).to(dev)
    tp[:nvoxel] = torch.from_numpy(t).to(dev)
    for nv in range(1, 9):
        got = _launch(Xp, tp, nvoxel, nv)
        assert np.all(np.isfinite(got)) and np.array_equal(got, ref[:nv]), nv
    # every column in every slot: rotate the columns
    for shift in range(1, 8):
        perm = [(j + shift) % 8 for j in range(8)]
        Xp[:, :nvoxel] = torch.from_numpy(X[perm]).to(dev)
        got = _launch(Xp, tp, nvoxel, 8)
        assert np.array_equal(got, ref[perm]), shift
    # a column alone in slot 0 with everything else NaN
    Xp[:] = float("nan")
    Xp[0, :nvoxel] = torch.from_numpy(X[5]).to(dev)
    assert np.array_equal(_launch(Xp, tp, nvoxel, 1)[0], ref[5])


@pytest.mark.parametrize("nvoxel", [65, 2049])
def test_special_truths(nvoxel):
    dev = torch.device("cuda", 0)
    X, t = _data(nvoxel, seed=2)
    Xd = torch.from_numpy(X).to(dev)
    # the dark frame: an all-zero truth
    z = np.zeros(nvoxel)
    got = _launch(Xd, torch.from_numpy(z).to(dev), nvoxel, 8)
    for j in range(8):
        check_sums(got[j], X[j], z, f"zero truth column {j}")
        assert got[j, 0] == 0 and got[j, 2] == 0 and got[j, 4] == 0 and got[j, 6] == 0 and got[j, 8] == 0
    # one non-zero voxel: s_in is that voxel of the column, exactly
    one = np.zeros(nvoxel)
    one[nvoxel - 2] = 3.5
    got = _launch(Xd, torch.from_numpy(one).to(dev), nvoxel, 8)
    for j in range(8):
        check_sums(got[j], X[j], one, f"one voxel column {j}")
        assert got[j, 6] == X[j, nvoxel - 2] and got[j, 0] == 3.5 and got[j, 2] == 12.25 and got[j, 8] == 3.5
        assert got[j, 4] == X[j, nvoxel - 2] * 3.5
    # x == t: s_dd and m_d exactly 0
    T = np.tile(t, (8, 1))
    got = _launch(torch.from_numpy(T).to(dev), torch.from_numpy(t).to(dev), nvoxel, 8)
    for j in range(8):
        check_sums(got[j], t, t, f"x == t column {j}")
        assert got[j, 5] == 0.0 and got[j, 7] == 0.0
        assert got[j, 0] == got[j, 1] == got[j, 6] and got[j, 2] == got[j, 3] == got[j, 4] and got[j, 8] == got[j, 9]


def test_launcher_refusals():
    from mpi_cuda_sartsolver_amd.ops import hip

    dev = torch.device("cuda", 0)
    b = torch.zeros(8 * 64, dtype=torch.float64, device=dev)
    s = torch.zeros(int(hip().phantom64_scratch_elems(64)), dtype=torch.float64, device=dev)
    for args, msg in [((b.data_ptr(), 64, 64, 0, b.data_ptr(), b.data_ptr(), s.data_ptr()), "nv = 0"),
                      ((b.data_ptr(), 64, 64, 9, b.data_ptr(), b.data_ptr(), s.data_ptr()), "nv = 9"),
                      ((b.data_ptr(), 63, 64, 1, b.data_ptr(), b.data_ptr(), s.data_ptr()), "must hold nvoxel"),
                      ((b.data_ptr(), 64, 0, 1, b.data_ptr(), b.data_ptr(), s.data_ptr()), "at least one voxel"),
                      ((0, 64, 64, 1, b.data_ptr(), b.data_ptr(), s.data_ptr()), "null operand")]:
        with pytest.raises(RuntimeError, match=msg):
            hip().phantom64(*args)
