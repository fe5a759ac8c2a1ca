"""The double-precision GPU path: the fp64 two-pass kernels (csrc/kernels/projection64.hip) against NumPy fp64 with
the bounds of the CPU kernels' tests (tests/test_cpu_solver.py), and ``SARTSolver(precision="fp64")`` (sart::Engine64)
against ``CPUSARTSolver`` with the same semantics flag: equal status and iteration count, solutions within
1e-9 max|x| (the project's fp64 bound; summation-order noise on these fixtures is ~4e-12 max|x|)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mpi_cuda_sartsolver_amd.models.cpu import CPUSARTSolver
from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams
from mpi_cuda_sartsolver_amd.utils.synthetic import host_problem

pytestmark = pytest.mark.gpu

# the smallest shapes with V % 4 != 0, a column block that is not full, fewer rows than splits, a ragged last split
SHAPES = [(1, 1), (7, 13), (300, 1001), (257, 4100), (2048, 4096)]
# a second split count per row count: more splits than rows (1, 7), ragged last splits (the others)
ODD_SPLITS = {1: 4, 7: 16, 300: 7, 257: 5, 2048: 37}
NAN = float("nan")


@pytest.fixture(scope="module")
def k():
    from mpi_cuda_sartsolver_amd.ops import hip

    return hip()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _shard(P, V):
    """(A, A fp64, device shard) of one shape: ld from choose_ld, nrows_pad a multiple of 64"""
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A = np.random.default_rng(1000 * P + V).random((P, V), dtype=np.float32)
    m = DenseRTM.from_dense(A, device=torch.device("cuda", 0))
    assert m.nrows_pad % 64 == 0 and m.ld % 64 == 0 and m.ld >= V
    return A, A.astype(np.float64), m


def _dvec(dev, n_pad, head, fill=0.0):
    """device fp64 vector of n_pad entries: `head`, then `fill`"""
    v = torch.full((n_pad,), fill, dtype=torch.float64, device=dev)
    v[:len(head)] = torch.from_numpy(np.asarray(head, dtype=np.float64))
    return v


def _forward(k, dev, m, P, V, epi, x, g, a, fill=0.0):
    xd, gd, ad = _dvec(dev, m.ld, x, fill), _dvec(dev, m.nrows_pad, g, fill), _dvec(dev, m.nrows_pad, a, fill)
    f = torch.full((m.nrows_pad,), fill, dtype=torch.float64, device=dev)
    w = torch.full((m.nrows_pad,), fill, dtype=torch.float64, device=dev)
    nb = k.forward_num_blocks(m.nrows_pad)
    Fp = torch.full((nb,), fill, dtype=torch.float64, device=dev)
    F = torch.full((1,), fill, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    k.forward64(epi, m.A.data_ptr(), m.ld, P, m.nrows_pad, V, xd.data_ptr(), gd.data_ptr(), ad.data_ptr(),
                f.data_ptr(), w.data_ptr(), Fp.data_ptr(), 0, s)
    k.sum_f64(Fp.data_ptr(), nb, F.data_ptr(), 0, s)
    torch.cuda.synchronize()
    return f[:P].cpu().numpy(), w[:P].cpu().numpy(), float(F.item())


def _backproject(k, dev, m, P, V, w, nsplit, fill=0.0):
    wd = _dvec(dev, m.nrows_pad, w, fill)
    part = torch.full((nsplit * m.ld,), fill, dtype=torch.float64, device=dev)
    out = torch.full((m.ld,), fill, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    k.backproject64(m.A.data_ptr(), m.ld, P, wd.data_ptr(), nsplit, part.data_ptr(), 0, s)
    k.reduce_partials_f64(part.data_ptr(), m.ld, nsplit, out.data_ptr(), s)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _operands(P, V):
    rng = np.random.default_rng(P + 7 * V)
    x, g = rng.random(V), rng.random(P) - 0.1
    a = np.where(rng.random(P) < 0.3, 0.0, rng.random(P))  # 30 % zero weights (masked / negative pixels)
    return x, g, a, rng.random(P) - 0.5


@pytest.mark.parametrize("P,V", SHAPES)
def test_forward64(k, dev, P, V):
    """f and sum f^2 to rtol 1e-12 (test_native_cpu_kernels' bounds). The weights are formed from f in one fp64
    operation each, so they inherit f's bound: |w - a (g - f_ref)| <= a |f - f_ref| + one rounding of the result
    <= 1e-12 a (|g| + |f_ref|) (linear), rtol 1e-12 (log); exactly 0 where a = 0."""
    A, A64, m = _shard(P, V)
    x, g, a, _ = _operands(P, V)
    fr = A64 @ x
    for epi in (0, 1, 2):
        f, w, F = _forward(k, dev, m, P, V, epi, x, g, a)
        np.testing.assert_allclose(f, fr, rtol=1e-12)
        assert np.isclose(F, np.sum(fr ** 2), rtol=1e-12), (F, np.sum(fr ** 2))
        if epi == 1:
            err = np.abs(w - a * (g - fr))
            print("forward64 linear w: max err / bound", np.max(err / np.maximum(1e-12 * a * (np.abs(g) + fr), 1e-300)))
            assert np.all(err <= 1e-12 * a * (np.abs(g) + np.abs(fr)))
            assert np.all(w[a == 0] == 0)
        if epi == 2:
            np.testing.assert_allclose(w, a * fr, rtol=1e-12)
            assert np.all(w[a == 0] == 0)


@pytest.mark.parametrize("P,V", SHAPES)
def test_backproject64(k, dev, P, V):
    A, A64, m = _shard(P, V)
    w = _operands(P, V)[3]  # signed
    ref = A64.T @ w
    for ns in (k.backproject_num_splits(m.ld, P), ODD_SPLITS[P]):
        out = _backproject(k, dev, m, P, V, w, ns)
        np.testing.assert_allclose(out[:V], ref, rtol=1e-10, atol=1e-12 * max(1.0, np.abs(w).sum()))
        assert np.all(out[V:] == 0)  # the padding columns of A are zero


@pytest.mark.parametrize("P,V", SHAPES)
def test_fp64_kernels_are_deterministic_and_ignore_padding(k, dev, P, V):
    """The same call twice gives identical bits; NaN in the padding of x (beyond V), of w / g / a (beyond P), in the
    outputs and the sum f^2 partials before the call, and in `partial` before the call changes no bit."""
    A, A64, m = _shard(P, V)
    x, g, a, w = _operands(P, V)
    for epi in (1, 2):
        r1 = _forward(k, dev, m, P, V, epi, x, g, a)
        r2 = _forward(k, dev, m, P, V, epi, x, g, a)
        r3 = _forward(k, dev, m, P, V, epi, x, g, a, fill=NAN)
        for u, v, t in zip(r1, r2, r3):
            assert np.array_equal(u, v) and np.array_equal(u, t) and np.all(np.isfinite(u))
    for ns in (k.backproject_num_splits(m.ld, P), ODD_SPLITS[P]):
        o1 = _backproject(k, dev, m, P, V, w, ns)
        o2 = _backproject(k, dev, m, P, V, w, ns)
        o3 = _backproject(k, dev, m, P, V, w, ns, fill=NAN)
        assert np.array_equal(o1, o2) and np.array_equal(o1, o3) and np.all(np.isfinite(o1))


# ------------------------------------------------------------------------------------ the solver against CpuSolver

FIXTURES = {
    # name: (host_problem arguments, Laplacian grid, parameters, expected (status, iterations) or None)
    "300x1001": ((300, 1001, 11), None, dict(max_iterations=60, conv_tolerance=1e-12), (-1, 60)),
    "2048x4096": ((2048, 4096, 9), None, dict(max_iterations=200, conv_tolerance=1e-7), None),
    "200x343-lap": ((200, 343, 11), (7, 7, 7), dict(max_iterations=60, conv_tolerance=1e-7, beta_laplace=2e-3), None),
}


@functools.lru_cache(maxsize=None)
def _problem(name):
    (P, V, seed), grid, kw, expect = FIXTURES[name]
    A, g, _ = host_problem(P, V, seed=seed, saturate_fraction=0.05)
    return A, g, (LaplacianCSR.grid_3d(*grid) if grid else None), kw, expect


@functools.lru_cache(maxsize=None)
def _cpu(name, log, semantics, tol_factor=1.0):
    """CpuSolver's result, computed once per case and shared (read-only)"""
    A, g, L, kw, _ = _problem(name)
    kw = dict(kw, conv_tolerance=kw["conv_tolerance"] * tol_factor)
    r = CPUSARTSolver(A, L, params=SolverParams(**kw), logarithmic=log, semantics=semantics).solve(g)
    r.solution.setflags(write=False)
    return r


def _gpu(name, log, semantics, dev, **kw):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, g, L, pkw, _ = _problem(name)
    s = SARTSolver(DenseRTM.from_dense(A, device=dev), L, params=SolverParams(**pkw), logarithmic=log,
                   precision="fp64", semantics=semantics, **kw)
    return s, g


def _close(x, ref):
    e = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
    print(f"max|x - x_ref| / max|x_ref| = {e:.3e}")
    return e <= 1e-9


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("semantics", ["gpu", "cpu"])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_fp64_solver_matches_cpu_solver(dev, name, semantics, log):
    ref = _cpu(name, log, semantics)
    expect = _problem(name)[4]
    if expect is not None:
        assert (ref.status, ref.iterations) == expect
    # precondition: the count is not on the stopping rule's edge (unchanged at 0.99 x and 1.01 x the tolerance)
    for fac in (0.99, 1.01):
        e = _cpu(name, log, semantics, fac)
        assert (e.status, e.iterations) == (ref.status, ref.iterations)
    s, g = _gpu(name, log, semantics, dev)
    assert type(s.engine).__name__ == "Engine64" and not s.use_fused
    r = s.solve(g)
    print(name, semantics, "log" if log else "linear", "status", r.status, "iterations", r.iterations)
    assert (r.status, r.iterations) == (ref.status, ref.iterations)
    assert r.used_fused is False and r.fused_variant == -1 and not r.nonfinite
    assert _close(r.solution, ref.solution)
    assert abs(r.convergence - ref.convergence) <= 1e-9 * max(1.0, abs(ref.convergence))


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("semantics", ["gpu", "cpu"])
def test_fp64_solver_warm_start(dev, semantics, log):
    """Solve, then a second measurement from the first solution: CpuSolver given the same x0."""
    name = "200x343-lap"
    A, g, L, kw, _ = _problem(name)
    s, _ = _gpu(name, log, semantics, dev)
    r1 = s.solve(g)
    g2 = np.where(g < 0, g, 1.07 * g + 0.01 * np.abs(g).max() * np.sin(np.arange(g.size)) ** 2)
    r2 = s.solve(g2, solution=r1.solution)
    c = CPUSARTSolver(A, L, params=SolverParams(**kw), logarithmic=log, semantics=semantics).solve(g2, solution=r1.solution)
    assert (r2.status, r2.iterations) == (c.status, c.iterations)
    assert _close(r2.solution, c.solution)
    assert not np.array_equal(r2.solution, r1.solution)


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
def test_fp64_check_interval_changes_nothing(dev, log):
    """The decision is the device's: reading the state every sweep or every 16 gives the same count and bits."""
    res = []
    for ci in (1, 16):
        s, g = _gpu("2048x4096", log, "gpu", dev, check_interval=ci)
        res.append(s.solve(g))
    assert (res[0].status, res[0].iterations) == (res[1].status, res[1].iterations)
    assert np.array_equal(res[0].solution, res[1].solution)


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
def test_fp64_solver_matches_torch_oracle(dev, log):
    """gpu semantics, tolerance 0, 20 updates: the fixed-count torch fp64 loop (models/oracle.py) on the same shard."""
    from mpi_cuda_sartsolver_amd.models.oracle import sart_oracle_f64
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, g, _, _, _ = _problem("2048x4096")
    m = DenseRTM.from_dense(A, device=dev)
    s = SARTSolver(m, None, params=SolverParams(max_iterations=20, conv_tolerance=0.0), logarithmic=log,
                   allow_zero_tolerance=True, precision="fp64", semantics="gpu")
    r = s.solve(g)
    assert (r.status, r.iterations) == (-1, 20)
    assert _close(r.solution, sart_oracle_f64(m, g, 20, logarithmic=log))


@pytest.mark.parametrize("semantics", ["gpu", "cpu"])
def test_fp64_nonfinite_conv_stops_the_frame(dev, semantics):
    """A NaN in the start value makes the first convergence metric non-finite: the frame stops there, as CpuSolver's
    (status -1, one update), and the result says so."""
    name = "200x343-lap"
    A, g, L, kw, _ = _problem(name)
    x0 = np.full(A.shape[1], 0.5)
    x0[17] = NAN
    s, _ = _gpu(name, False, semantics, dev)
    r = s.solve(g, solution=x0)
    c = CPUSARTSolver(A, L, params=SolverParams(**kw), semantics=semantics).solve(g, solution=x0)
    assert (c.status, c.iterations) == (-1, 1)
    assert (r.status, r.iterations) == (c.status, c.iterations) and r.nonfinite and not np.isfinite(r.convergence)
    good = s.solve(g)  # the engine is usable afterwards
    assert not good.nonfinite and _close(good.solution, _cpu(name, False, semantics).solution)


def test_fp64_refusals(dev):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM, SparseRTM

    A, g, _ = host_problem(96, 200, seed=3)
    m = DenseRTM.from_dense(A, device=dev)
    with pytest.raises(ValueError, match="bf16"):
        SARTSolver(m.to_bf16(), precision="fp64")
    with pytest.raises(ValueError, match="f16"):
        SARTSolver(m.to_f16(), precision="fp64")
    with pytest.raises(ValueError, match="sparse"):
        SARTSolver(SparseRTM.from_dense(A, device=dev), precision="fp64")
    with pytest.raises(ValueError, match="column"):
        SARTSolver(m, precision="fp64", partition="cols")
    with pytest.raises(ValueError, match="fused"):
        SARTSolver(m, precision="fp64", use_fused=True)
    with pytest.raises(ValueError, match="precision"):
        SARTSolver(m, precision="fp16")
    with pytest.raises(ValueError, match="semantics"):
        SARTSolver(m, precision="fp64", semantics="reference")
    with pytest.raises(ValueError, match="semantics"):
        SARTSolver(m, semantics="cpu")  # the fp32 engine has one


def test_fp32_precision_still_builds_the_fp32_engine(dev):
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM

    A, g, _ = host_problem(512, 2048, seed=1)  # the smoke run's shape: the fused sweep
    m = DenseRTM.from_dense(A, device=dev)
    for s in (SARTSolver(m), SARTSolver(m, precision="fp32")):
        assert type(s.engine).__name__ == "Engine" and s.use_fused and s.precision == "fp32"
        assert s.solve(g).used_fused
    assert type(SARTSolver(m, precision="fp64").engine).__name__ == "Engine64"
