"""Multi-frame MFMA solver vs the per-frame fp64 oracle of the GPU semantics: statuses and iteration counts of the
tolerance-stopped runs, and solutions at the fp32-emulation bound (tests/fp32_bound.py: no further from the oracle,
after the frame's own update count, than an fp32 evaluation of the same chain)."""
import numpy as np
import pytest
from fp32_bound import check_fp32_bound

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("nframes,batch", [(1, 16), (5, 16), (16, 16), (19, 16), (27, 32), (40, 64)])
def test_multiframe_vs_oracle(log, nframes, batch):
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(nframes)
    P, V = 700, 1000
    A = rng.random((P, V), dtype=np.float32)
    X = rng.random((nframes, V)) + 0.05
    G = X @ A.T.astype(np.float64)
    G[rng.random(G.shape) < 0.03] = -1.0
    L = LaplacianCSR.grid_3d(10, 10, 10, device=dev)
    kw = dict(max_iterations=40, conv_tolerance=1e-4, beta_laplace=1e-3)
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), L, None, SolverParams(**kw), logarithmic=log,
                             batch=batch)
    assert s.batch_width == batch
    res = s.solve_batch(G)
    assert len(res) == nframes
    for f in range(nframes):
        x, st, it = sart_gpu_semantics(A, G[f], L, logarithmic=log, **kw)
        assert res[f].status == st
        assert abs(res[f].iterations - it) <= 2
    for f in sorted({0, nframes // 2, nframes - 1}):
        check_fp32_bound(res[f].solution, A, G[f], L, log=log, iterations=res[f].iterations, beta_laplace=1e-3)


def check_chain_provenance(res, starts, stats, A, G, L, x0, log, kw):
    """Every frame of a chained series: its recorded start value is its named source (warm_from after warm_iter
    updates: x0, a finished frame's solution rescaled bitwise, or the oracle's iterate of a frame in flight at the
    oracle's fp32 drift), and the frame matches the oracle started from that value (status, iterations, and every
    seventh frame's solution at the fp32 bound)."""
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics

    nframes = len(res)
    norm = G.max(axis=1)
    for f in range(nframes):
        wf, wi = res[f].warm_from, res[f].warm_iter
        if wf < 0:
            src = x0
        elif not res[f].warm_live:  # the source had finished: its solution, rescaled (bitwise)
            assert wi == res[wf].iterations
            src = res[wf].solution
        else:  # in flight: the oracle's iterate of the source after wi updates from its own recorded start,
            # extrapolated along its last update in linear mode (x + c (x - x_prev), MfQueue::src_extrap)
            def it(n):
                return sart_gpu_semantics(A, G[wf], L, logarithmic=log, x_prev=starts[wf],
                                          **dict(kw, max_iterations=n, conv_tolerance=0.0))[0]
            src = it(wi)
            c = 0.0 if log else stats["src_extrap"]
            if c:
                src = src + c * (src - it(wi - 1))
            assert wi >= stats["src_age"]
        want = np.maximum((src / norm[f]).astype(np.float32), np.float32(1e-7))
        got = (starts[f] / norm[f]).astype(np.float32)
        if wf < 0 or not res[f].warm_live:
            np.testing.assert_array_equal(got, want)
        else:
            assert np.linalg.norm(got - want) <= 1e-3 * np.linalg.norm(want), f
        x, st, it = sart_gpu_semantics(A, G[f], L, logarithmic=log, x_prev=starts[f], **kw)
        assert res[f].status == st and abs(res[f].iterations - it) <= 2, (f, res[f].iterations, it)
        if f % 7 == 0 or f == nframes - 1:
            check_fp32_bound(res[f].solution, A, G[f], L, log=log, iterations=res[f].iterations, beta_laplace=1e-3,
                             x_prev=starts[f])


@pytest.mark.parametrize("log", [False, True])
def test_multiframe_warm_chain(log):
    """Time series with device-side refill: the first frames start from x0, every later frame from the current
    iterate of the newest frame in flight (with >= src_age updates) or finished (warm_from, with warm_iter updates),
    rescaled to its own normalisation. Each frame matches the oracle started from its recorded start value; each start value is the
    source's iterate (bitwise when the source had finished, at the oracle's fp32 drift when it was in flight).
    Frames converge after different iteration counts, so slots are refilled at different sweeps."""
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    P, V, nframes, batch = 600, 1000, 40, 16
    A = rng.random((P, V), dtype=np.float32)
    base = rng.random(V) + 0.1
    # a varying series: some frames close to their predecessor, some far (different iteration counts)
    X = base[None] * (1.0 + rng.choice([0.01, 0.3], size=(nframes, 1)) * rng.random((nframes, V)))
    G = X @ A.T.astype(np.float64)
    L = LaplacianCSR.grid_3d(10, 10, 10, device=dev)
    kw = dict(max_iterations=60, conv_tolerance=1e-5, beta_laplace=1e-3)
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), L, None, SolverParams(**kw), logarithmic=log,
                             batch=batch)
    x0 = base * 1.5
    res = s.solve_batch(G, x0=x0, chain=True, record_starts=True)
    starts, stats = s.starts, s.series_stats
    cap = stats["admit_cap"]
    assert 1 <= cap < batch and stats["frames"] == nframes and 0 < stats["slot_util"] <= 1.0
    assert all(res[f].warm_from == -1 for f in range(cap))
    # until a frame in flight has src_age updates the new frames start from x0 too; every later one is chained
    assert all(res[f].warm_from < f for f in range(nframes))
    first = min(f for f in range(nframes) if res[f].warm_from >= 0)
    assert first <= cap * (stats["src_age"] + 1) and all(res[f].warm_from >= 0 for f in range(first, nframes))
    assert len({res[f].iterations for f in range(nframes)}) > 1  # slots really refill at different sweeps
    assert any(res[f].warm_live for f in range(nframes))  # sources in flight
    check_chain_provenance(res, starts, stats, A, G, L, x0, log, kw)
    # without chain, every frame after the first batch cold-starts even when x0 is given
    cold = s.solve_batch(G[:20], x0=x0)
    assert all(r.warm_from == -1 for r in cold)
    x, st, it = sart_gpu_semantics(A, G[17], L, logarithmic=log, **kw)
    assert cold[17].status == st
    check_fp32_bound(cold[17].solution, A, G[17], L, log=log, iterations=cold[17].iterations, beta_laplace=1e-3)
    x, st, it = sart_gpu_semantics(A, G[3], L, logarithmic=log, x_prev=x0, **kw)  # the first batch: from x0
    assert cold[3].status == st and abs(cold[3].iterations - it) <= 2


@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("log", [False, True])
def test_multiframe_warm_chain_starved(monkeypatch, log, w):
    """SART_MF_STAGE_WINDOW=w: entry e is staged only once e < finished + w, so the queue starves whatever the host's
    timing: slots drain, plans run alone and refill from the newest finished solution on the device. Every frame
    keeps the provenance of the chained series; with w = 1 the batched engine is the sequential warm-start chain:
    frame f starts from frame f - 1's solution, rescaled bitwise, and matches the oracle started from the oracle's
    previous solution at the fp32 bound of that chain (the emulation chained like the run; restarted from the fp64
    solution at every frame it leaves out what a chain accumulates: measured on this series, linear e grows from
    6.7e-8 at frame 0 to 2.5e-7 at frame 22 against a restarted e32 of 5.5e-8, log e is 3.7e-6 from frame 1 on
    against 3.6e-7, the sequential single-frame engine's chain shows the same, 2.3e-7 and 3.5e-6, and the chained emulation 2.4e-7
    and 6.5e-6)."""
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    monkeypatch.setenv("SART_MF_STAGE_WINDOW", str(w))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    P, V, nframes, batch = 600, 1000, 24, 16
    A = rng.random((P, V), dtype=np.float32)
    base = rng.random(V) + 0.1
    X = base[None] * (1.0 + rng.choice([0.01, 0.3], size=(nframes, 1)) * rng.random((nframes, V)))
    G = X @ A.T.astype(np.float64)
    L = LaplacianCSR.grid_3d(10, 10, 10, device=dev)
    kw = dict(max_iterations=60, conv_tolerance=1e-5, beta_laplace=1e-3)
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), L, None, SolverParams(**kw), logarithmic=log,
                             batch=batch)
    x0 = base * 1.5
    res = s.solve_batch(G, x0=x0, chain=True, record_starts=True)
    starts, stats = s.starts, s.series_stats
    assert stats["stage_window"] == w and stats["frames"] == nframes
    assert all(res[f].warm_from < f for f in range(nframes))
    check_chain_provenance(res, starts, stats, A, G, L, x0, log, kw)
    if w != 1:
        return
    from fp32_bound import ORDERS, rel
    from mpi_cuda_sartsolver_amd.models.reference import sart_fp32_emulation

    norm = G.max(axis=1)
    assert res[0].warm_from == -1
    # The sequential chain of the oracle itself: each frame from the oracle's previous solution (frame 0 from x0), run
    # for our recorded update count. Bounded as check_fp32_bound bounds one frame (factor 1, slack 1e-7), by the fp32
    # emulation of the same chain: the emulation starts each frame from its own previous solution, as every fp32
    # solver of a sequential series must (tests/test_cli_e2e.py chain_errors(warm=True) bounds the sequential mode
    # this way); restarted from the fp64 solution at every frame it would leave out what any fp32 chain accumulates.
    prev64, prev32 = x0, {o: x0 for o in ORDERS}
    for f in range(nframes):
        if f >= 1:
            assert res[f].warm_from == f - 1 and not res[f].warm_live, (f, res[f].warm_from, res[f].warm_live)
            want = np.maximum((res[f - 1].solution / norm[f]).astype(np.float32), np.float32(1e-7))
            np.testing.assert_array_equal((starts[f] / norm[f]).astype(np.float32), want)
        okw = dict(logarithmic=log, max_iterations=res[f].iterations, beta_laplace=1e-3)
        prev64 = sart_gpu_semantics(A, G[f], L, x_prev=prev64, conv_tolerance=0.0, **okw)[0]
        prev32 = {o: sart_fp32_emulation(A, G[f], L, x_prev=prev32[o], order=o, **okw)[0] for o in ORDERS}
        e, e32 = rel(res[f].solution, prev64), max(rel(prev32[o], prev64) for o in ORDERS)
        assert e <= e32 + 1e-7, f"frame {f}: rel {e:.3e} vs the fp32 emulation of the chain {e32:.3e}"

def test_multiframe_series_iterations_near_sequential():
    """A slowly drifting series (the ray-traced phantom's regime): the pipelined chain keeps the warm start's
    iteration savings -- mean iterations per frame within 2x of the frame-by-frame chain's -- and the slots stay
    busy (the plan admits in the sweep a frame finishes)."""
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SARTSolver, SolverParams

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    P, V, nframes = 1500, 1200, 96
    A = rng.random((P, V), dtype=np.float32)
    b = rng.random(V) + 0.5
    ph = 2 * np.pi * rng.random(V)
    X = np.stack([b * (1 + 0.05 * np.sin(2 * np.pi * t / 200.0 + ph)) for t in range(nframes)])
    G = X @ A.T.astype(np.float64)
    kw = dict(max_iterations=400, conv_tolerance=1e-7)
    rtm = DenseRTM.from_dense(A, device=dev)
    seq = SARTSolver(rtm, None, None, SolverParams(**kw))
    its, prev = [], None
    for f in range(nframes):
        r = seq.solve(G[f], prev)
        its.append(r.iterations)
        prev = r.solution
    mf = MultiFrameSARTSolver(rtm, None, None, SolverParams(**kw), batch=32)
    res = mf.solve_batch(G, chain=True)
    mean_b, mean_s = np.mean([r.iterations for r in res]), np.mean(its[1:])
    assert all(r.status == 0 for r in res)
    assert mean_b <= 2.0 * mean_s + 1.0, (mean_b, mean_s, mf.series_stats)
    # (96 frames of ~4 sweeps each: admission ramp and drain are a large share of so short a series)
    assert mf.series_stats["slot_util"] > 0.3, mf.series_stats


def test_multiframe_drift_starts(monkeypatch):
    """SART_MF_DRIFT=1 (MfQueue::drift): on a linearly drifting series a chained frame's start adds the frame gap to
    its source times the per-frame change between the two newest finished solutions. Every frame still solves to
    the oracle from its recorded start, and the starts land nearer the frames' own solutions than without the drift."""
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    P, V, nframes = 800, 1000, 64
    A = rng.random((P, V), dtype=np.float32)
    b, d = rng.random(V) + 0.5, 0.01 * (rng.random(V) - 0.5)
    X = np.stack([b + t * d for t in range(nframes)])
    G = X @ A.T.astype(np.float64)
    kw = dict(max_iterations=300, conv_tolerance=1e-5)  # (the reference default; fp32 sums stall near 1e-7)
    rtm = DenseRTM.from_dense(A, device=dev)
    out = {}
    for drift in ("0", "1"):
        monkeypatch.setenv("SART_MF_DRIFT", drift)
        s = MultiFrameSARTSolver(rtm, None, None, SolverParams(**kw), batch=16)
        res = s.solve_batch(G, chain=True, record_starts=True)
        assert s.series_stats["drift"] == float(drift)
        assert all(r.status == 0 for r in res)
        out[drift] = (res, s.starts.copy())
    res, starts = out["1"]
    chained = [f for f in range(nframes) if res[f].warm_from >= 0]
    assert len(chained) > nframes // 2
    for f in chained[::7]:
        x, st, it = sart_gpu_semantics(A, G[f], None, x_prev=starts[f], **kw)
        assert res[f].status == st and abs(res[f].iterations - it) <= 2, (f, res[f].iterations, it)
    late = range(nframes // 2, nframes)  # (xlast and xlast2 both exist by then)
    dist = {k: np.mean([np.linalg.norm(v[1][f] - v[0][f].solution) / np.linalg.norm(v[0][f].solution) for f in late])
            for k, v in out.items()}
    assert any(not np.array_equal(out["0"][1][f], starts[f]) for f in late)
    assert dist["1"] < dist["0"], dist


@pytest.mark.parametrize("log", [False, True])
def test_multiframe_nonfinite_slot_is_rolled_back_and_refilled(monkeypatch, log):
    """A NaN injected into slot 0's iterate after sweep 5 (SART_FAULT_NAN) stops that frame at the next sweep:
    it returns its last finite iterate (5 updates, flagged non-finite) while the other frames continue, and the
    slot takes the next frame of the queue, which solves normally."""
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.reference import sart_gpu_semantics
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    monkeypatch.setenv("SART_FAULT_NAN", "5")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    P, V, nframes = 500, 800, 20
    A = rng.random((P, V), dtype=np.float32)
    G = (rng.random((nframes, V)) + 0.05) @ A.T.astype(np.float64)
    kw = dict(max_iterations=30, conv_tolerance=0.0)  # every frame runs 30 sweeps: slot 0 is live at sweep 5
    s = MultiFrameSARTSolver(DenseRTM.from_dense(A, device=dev), None, None, SolverParams(**kw), logarithmic=log,
                             batch=16, allow_zero_tolerance=True)
    res = s.solve_batch(G)
    assert res[0].nonfinite and res[0].iterations == 5 and np.all(np.isfinite(res[0].solution))
    check_fp32_bound(res[0].solution, A, G[0], None, log=log, iterations=5)
    for f in range(1, nframes):
        assert not res[f].nonfinite
        x, st, it = sart_gpu_semantics(A, G[f], None, logarithmic=log, **kw)
        assert res[f].status == st and abs(res[f].iterations - it) <= 2, (f, res[f].iterations, it)
    for f in (1, 16, nframes - 1):  # frame 16: the refill of the rolled-back slot
        check_fp32_bound(res[f].solution, A, G[f], None, log=log, iterations=res[f].iterations)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("tol", [0.0, 1e-4])
def test_final_sweep_skips_backprojection_bitwise(monkeypatch, log, tol):
    """The batch's final sweep (every running frame decided at max_iter) runs the forward and the decision only;
    its back-projection and update would be discarded. Solutions, iteration counts, statuses and convergence
    values equal those of SART_MF_LAST_BWD=1 (the full final sweep) bit for bit, with slots refilled across chunk
    boundaries (40 frames through 16 slots, chunks of 5 sweeps)."""
    from mpi_cuda_sartsolver_amd.models.laplacian import LaplacianCSR
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    P, V, nframes = 600, 1000, 40
    A = rng.random((P, V), dtype=np.float32)
    G = (rng.random((nframes, V)) + 0.05) @ A.T.astype(np.float64)
    L = LaplacianCSR.grid_3d(10, 10, 10, device=dev)
    rtm = DenseRTM.from_dense(A, device=dev)
    out = {}
    for full in ("1", "0"):
        monkeypatch.setenv("SART_MF_LAST_BWD", full)
        s = MultiFrameSARTSolver(rtm, L, None, SolverParams(max_iterations=12, conv_tolerance=tol, beta_laplace=1e-3),
                                 logarithmic=log, batch=16, check_interval=5, allow_zero_tolerance=True)
        out[full] = s.solve_batch(G)
        del s
    for a, b in zip(out["1"], out["0"]):
        assert (a.status, a.iterations, a.convergence, a.nonfinite) == (b.status, b.iterations, b.convergence,
                                                                        b.nonfinite)
        assert np.array_equal(a.solution, b.solution)
    if tol == 0.0:  # fixed iteration count: every frame reaches the final-sweep decision
        assert all(r.iterations == 12 for r in out["0"])


@pytest.mark.parametrize("storage,batch,split_a", [("bf16", 32, None), ("fp32", 64, True)])
def test_engine_plans_once(monkeypatch, storage, batch, split_a):
    """The engine takes its launch plans (kernel variants, split counts, chunk alignment) at construction: tile and
    split-count knobs set in the process afterwards change nothing. Six runs of 3 sweeps each on one engine, every run
    started from frame 0's previous iterate, the knobs set after the third: all six iterates equal, bit for bit, those
    of an engine that never saw the knobs. 2048 columns make VT = 2 the bf16 default (a tile re-derived per launch
    would change the kernel and the partial slices); 1000 rows exercise the padded tail."""
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    knobs = {"SART_MF_B16_VT": "1", "SART_MF_X3_VT": "2", "SART_MF_X3_FWD": "4,2", "SART_MF_BP_BLOCKS": "64"}
    for name in knobs:
        monkeypatch.delenv(name, raising=False)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(batch)
    P, V = 1000, 2048
    A = rng.random((P, V), dtype=np.float32)
    rtm = DenseRTM.from_dense(A, device=dev, storage=storage)
    G = (rng.random((batch, V)) + 0.05) @ A.T.astype(np.float64)

    def engine():
        s = MultiFrameSARTSolver(rtm, None, None, SolverParams(max_iterations=3, conv_tolerance=0.0), batch=batch,
                                 allow_zero_tolerance=True, split_a=split_a)
        assert s.batch_width == batch and s.split_a == bool(split_a)
        return s

    def run(s, x0):
        return np.stack([r.solution for r in s.solve_batch(G, x0=x0)])

    ref, x0 = [], None
    s = engine()
    for _ in range(6):
        ref.append(run(s, x0))
        x0 = ref[-1][0]
    del s
    s, x0 = engine(), None
    for i in range(6):
        if i == 3:
            for name, val in knobs.items():
                monkeypatch.setenv(name, val)
        x = run(s, x0)
        assert np.array_equal(x, ref[i]), i
        x0 = x[0]
    assert not np.array_equal(ref[0], ref[5])


@pytest.fixture(scope="module")
def plan_shard():
    rng = np.random.default_rng(7)
    return rng.random((700, 1000), dtype=np.float32)


@pytest.mark.parametrize("storage,batch,env", [
    ("fp32", 16, {}),
    ("fp32", 32, {}),
    ("fp32", 64, {"SART_MF_FWD16": "0", "SART_MF_BWD16": "0"}),
    ("bf16", 128, {}),
    ("f16", 128, {}),
    ("sparse", 128, {}),
])
def test_engine_holds_the_plan(monkeypatch, plan_shard, storage, batch, env):
    """A live engine's plan is mf_engine_plan() of the same shard, configuration and environment, and the accessors
    and the series statistics read it (700 x 1000, ld 1024; every storage, the split-A default and both bf16-piece
    paths)."""
    from mpi_cuda_sartsolver_amd.models.multiframe import MultiFrameSARTSolver
    from mpi_cuda_sartsolver_amd.models.rtm import DenseRTM, SparseRTM
    from mpi_cuda_sartsolver_amd.models.sart import SolverParams

    for name in ("SART_MF_X3", "SART_MF_FWD16", "SART_MF_BWD16", "SART_MF_XBLK", "SART_MF_SPARSE_PW", "SART_MF_CHUNK"):
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    dev = torch.device("cuda", 0)
    A = plan_shard
    rtm = SparseRTM.from_dense(A, device=dev) if storage == "sparse" else DenseRTM.from_dense(A, device=dev,
                                                                                                storage=storage)
    s = MultiFrameSARTSolver(rtm, None, None, SolverParams(max_iterations=3, conv_tolerance=0.0), batch=batch,
                             check_interval=5, allow_zero_tolerance=True)
    e, k = s.engine, s.k
    sparse = storage == "sparse"
    want = k.mf_engine_plan({"fp32": "f32", "sparse": "f32"}.get(storage, storage), sparse,
                            int(rtm.nnz) if sparse else 0, batch, 700, 704, 1024, ranks=1, mf_split_a=-1,
                            check_interval=5)
    plan = e.plan
    assert plan == want
    names = {("fp32", 16): ("fp32", "fp32"), ("fp32", 32): ("f16x2", "f16x2"), ("fp32", 64): ("bf16x2", "bf16x3"),
             ("bf16", 128): ("bf16-storage",) * 2, ("f16", 128): ("f16-storage",) * 2,
             ("sparse", 128): ("sparse-fp32",) * 2}[storage, batch]
    assert (e.batch_frames, e.sparse) == (plan["nf"], plan["sparse"]) == (batch, sparse)
    assert e.split_a == plan["split_a"] == (storage == "fp32" and batch >= 32)
    assert (e.forward_split, e.backproject_split) == (plan["forward_split"], plan["backproject_split"]) == names
    assert (s.batch_width, s.split_a, s.forward_split, s.backproject_split) == (batch, e.split_a, *names)
    G = (np.random.default_rng(1).random((3, 1000)) + 0.05) @ A.T.astype(np.float64)
    for chain in (False, True):
        assert all(r.iterations == 3 for r in s.solve_batch(G, chain=chain))
        st = s.series_stats
        assert (st["chunk"], st["src_age"], st["src_finished"], st["src_extrap"], st["stage_window"]) == (
            plan["chunk"], plan["src_age"], plan["src_finished"], plan["src_extrap"], plan["stage_window"])
        assert (st["admit_cap"], st["drift"], st["lead"]) == (
            (plan["admit_cap"], plan["drift"], plan["lead"]) if chain else (0, 0.0, False))
