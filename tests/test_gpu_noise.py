"""The noise kernel (csrc/kernels/noise.hip) against the NumPy restatement of the noise definition
(utils/philox.py::perturb): every element within 1e-12 (|g| + sigma (1 + |z|)) -- the device's log, cos and sqrt against
NumPy's are a few ulp apart, and the words of the generator are integers, so exact --, at sizes around the 64-pixel
padding and the 256-thread workgroup, in the first and in a second chunk of replicas, at pixel indices up to 2^32, for
each noise term alone and all three; padding untouched, runs bitwise repeatable, and a rank's slice carrying the bits
of the whole frame's call."""
import itertools

import numpy as np
import pytest

from mpi_cuda_sartsolver_amd.utils import philox

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TIME, SEED = 0.125, 0x123456789ABCDEF0
TERMS = {"abs": (0.05, 0.0, 0.0), "shot": (0.0, 0.01, 0.0), "rel": (0.0, 0.0, 0.02), "all": (0.05, 0.01, 0.02)}
RMAX = 65 + 17 - 1  # the last replica any case asks for


@pytest.fixture(scope="module")
def k():
    from mpi_cuda_sartsolver_amd.ops import hip

    return hip()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _frame(n):
    g = np.random.default_rng(n).uniform(0.0, 2.0, n)
    g[::5] = -1.0     # excluded
    g[1::7] = 0.0     # dark
    g[2::9] = 1e-6    # clamped at 0 about half of the time
    return g


def _call(k, dev, g, pixel0, r0, nrep, terms, seed=SEED, time=TIME):
    n = g.size
    ldo = (n + 63) // 64 * 64
    gd = torch.from_numpy(g).to(dev)
    out = torch.full((nrep, ldo), float("nan"), dtype=torch.float64, device=dev)
    k.noise_replicas(gd.data_ptr(), n, pixel0, philox.time_bits(time), r0, nrep, *terms, seed, out.data_ptr(), ldo,
                     torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_noise_replicas_against_perturb(k, dev, n):
    g = _frame(n)
    worst = 0.0
    for pixel0, (name, terms) in itertools.product((0, 4_000_000_000), TERMS.items()):
        ref = philox.perturb(g, TIME, RMAX, *terms, seed=SEED, pixel0=pixel0)
        sigma = np.where(g < 0, 0.0, philox.noise_sigma(np.abs(g), *terms))
        pixels = np.arange(n, dtype=np.uint64) + np.uint64(pixel0)
        for r0, nrep in itertools.product((1, 65), (1, 3, 17)):
            out = _call(k, dev, g, pixel0, r0, nrep, terms)
            assert np.all(np.isnan(out[:, n:])), "padding written"
            for i in range(nrep):
                z = philox.noise_normals(SEED, TIME, pixels, r0 + i)
                tol = 1e-12 * (np.abs(g) + sigma * (1.0 + np.abs(z)))
                err = np.abs(out[i, :n] - ref[r0 + i])
                assert np.all(err <= tol), (name, pixel0, r0, nrep, i, float(err.max()))
                worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
                assert np.array_equal(out[i, :n][g < 0], g[g < 0]) and np.all(out[i, :n][g >= 0] >= 0.0)
    print(f"n={n}: worst error / tolerance {worst:.3e}")


def test_replica_zero_is_the_frame(k, dev):
    g = _frame(65)
    out = _call(k, dev, g, 0, 0, 2, TERMS["all"])
    assert np.array_equal(out[0, :65], g)
    assert np.array_equal(out[1, :65], _call(k, dev, g, 0, 1, 1, TERMS["all"])[0, :65])


def test_same_call_twice_gives_identical_bits(k, dev):
    g = _frame(1000)
    a, b = (_call(k, dev, g, 7, 1, 17, TERMS["all"]) for _ in range(2))
    assert np.array_equal(a[:, :1000], b[:, :1000])
    # and every coordinate matters
    for other in (_call(k, dev, g, 8, 1, 17, TERMS["all"]), _call(k, dev, g, 7, 2, 17, TERMS["all"]),
                  _call(k, dev, g, 7, 1, 17, TERMS["all"], seed=SEED + 1),
                  _call(k, dev, g, 7, 1, 17, TERMS["all"], time=-TIME)):
        assert not np.array_equal(other[:, :1000], a[:, :1000])


@pytest.mark.parametrize("n", [64, 1000])
def test_two_half_range_calls_concatenate_to_the_full_call(k, dev, n):
    """The rank-invariance property: a rank passes its first pixel's global index."""
    g = _frame(n)
    h = n // 2
    full = _call(k, dev, g, 0, 1, 17, TERMS["all"])[:, :n]
    lo = _call(k, dev, g[:h].copy(), 0, 1, 17, TERMS["all"])[:, :h]
    hi = _call(k, dev, g[h:].copy(), h, 1, 17, TERMS["all"])[:, : n - h]
    assert np.array_equal(np.concatenate([lo, hi], axis=1), full)


def test_refusals(k, dev):
    g = torch.zeros(64, dtype=torch.float64, device=dev)
    out = torch.zeros((65, 64), dtype=torch.float64, device=dev)
    bits = philox.time_bits(TIME)
    for n, pixel0, nrep, terms, ldo in ((64, 0, 65, (1.0, 0.0, 0.0), 64), (64, 0, 0, (1.0, 0.0, 0.0), 64),
                                        (64, 2 ** 32 - 63, 1, (1.0, 0.0, 0.0), 64), (64, 0, 1, (-1.0, 0.0, 0.0), 64),
                                        (64, 0, 1, (1.0, 0.0, 0.0), 63)):
        with pytest.raises(RuntimeError, match="noise_replicas"):
            k.noise_replicas(g.data_ptr(), n, pixel0, bits, 1, nrep, *terms, 0, out.data_ptr(), ldo, 0)


def test_perturbed_frames_api(dev):
    from mpi_cuda_sartsolver_amd.models.uncertainty import perturbed_frames

    g = _frame(300)
    out = perturbed_frames(g, TIME, 70, *TERMS["all"], seed=SEED, pixel0=100, device=dev)  # two chunks
    ref = philox.perturb(g, TIME, 70, *TERMS["all"], seed=SEED, pixel0=100)
    assert out.shape == (71, 300) and np.array_equal(out[0], g)
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-12 * 4.0)  # |g| + sigma (1 + |z|) < 4 on this frame
