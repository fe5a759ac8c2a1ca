"""The noise definition of --replicas on the host: Philox4x32-10's known answers through the NumPy emulation
(utils/philox.py) and through the native binding (csrc/kernels/philox.hpp, the text the noise kernel compiles), the two
against each other word for word, the normals' moments, and what `perturb` promises."""
import itertools

import numpy as np
import pytest

from mpi_cuda_sartsolver_amd.ops import native
from mpi_cuda_sartsolver_amd.utils import philox

KNOWN = [  # counter, key, output: the Random123 known-answer vectors of philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
PIXELS = [0, 1, 2 ** 32 - 1]
REPLICAS = [1, 1024]
TIMES = [0.0, -0.0, 0.125]
SEEDS = [0, 2 ** 64 - 1]


@pytest.mark.parametrize("counter, key, out", KNOWN)
def test_known_answers_emulation(counter, key, out):
    assert tuple(int(w) for w in philox.philox4x32_10(counter, key)) == out


@pytest.mark.parametrize("counter, key, out", KNOWN)
def test_known_answers_binding(counter, key, out):
    assert tuple(native().philox4x32_10(list(counter), list(key))) == out


def _binding_words(seed, time, pixel, replica):
    bits = philox.time_bits(time)
    return tuple(native().philox4x32_10([pixel, replica, bits & 0xffffffff, bits >> 32],
                                        [seed & 0xffffffff, seed >> 32]))


def test_emulation_and_binding_agree_on_the_words():
    streams = {}
    for seed, time, replica in itertools.product(SEEDS, TIMES, REPLICAS):
        emu = philox.noise_words(seed, time, PIXELS, replica)
        for i, pixel in enumerate(PIXELS):
            words = _binding_words(seed, time, pixel, replica)
            assert tuple(int(w) for w in emu[i]) == words, (seed, time, pixel, replica)
            streams[(seed, philox.time_bits(time), pixel, replica)] = words
    # 0.0 and -0.0 differ in their bits, so in their streams; and no two of the 36 counters collide
    assert philox.time_bits(0.0) != philox.time_bits(-0.0)
    assert len(set(streams.values())) == len(SEEDS) * len(TIMES) * len(REPLICAS) * len(PIXELS)
    for seed, pixel, replica in itertools.product(SEEDS, PIXELS, REPLICAS):
        assert streams[(seed, philox.time_bits(0.0), pixel, replica)] != \
            streams[(seed, philox.time_bits(-0.0), pixel, replica)]


def test_noise_normal_matches_the_emulation():
    n = native()
    pixels = np.concatenate([np.arange(4096, dtype=np.uint64), np.array(PIXELS, dtype=np.uint64)])
    worst = 0.0
    for seed, time, replica in itertools.product(SEEDS, TIMES, REPLICAS):
        ref = philox.noise_normals(seed, time, pixels, replica)
        z = np.asarray(n.noise_normals(seed, time, pixels.astype(np.uint32), replica))
        err = np.abs(z - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1e-12), (seed, time, replica, float(err.max()))
        assert n.noise_normal(seed, time, int(pixels[-1]), replica) == z[-1]  # the scalar form: the same function
    print(f"noise_normal against the emulation: worst |dz| / max(1, |z|) = {worst:.3e}")


def test_moments_of_the_normals():
    z = philox.noise_normals(0, 0.125, np.arange(2 ** 20, dtype=np.uint64), 1)
    mean, std, m4 = float(z.mean()), float(z.std()), float(np.mean(z ** 4))
    print(f"2^20 normals: mean {mean:.3e} std {std:.5f} fourth moment {m4:.4f} max |z| {np.abs(z).max():.3f}")
    assert np.all(np.isfinite(z))
    assert abs(mean) <= 5e-3 and abs(std - 1.0) <= 5e-3  # five standard errors of either (1e-3 and 7e-4)


def test_every_coordinate_changes_the_stream():
    pixels = np.arange(64, dtype=np.uint64)
    base = philox.noise_normals(7, 1.5, pixels, 3)
    assert np.array_equal(base, philox.noise_normals(7, 1.5, pixels, 3))
    for other in (philox.noise_normals(8, 1.5, pixels, 3), philox.noise_normals(7 + 2 ** 32, 1.5, pixels, 3),
                  philox.noise_normals(7, np.nextafter(1.5, 2.0), pixels, 3), philox.noise_normals(7, 1.5, pixels, 4),
                  philox.noise_normals(7, 1.5, pixels + np.uint64(64), 3)):
        assert not np.any(other == base)
    # a pixel's value depends on its global index alone: a slice of the range carries the whole range's bits
    assert np.array_equal(philox.noise_normals(7, 1.5, pixels[32:], 3), base[32:])


def test_perturb():
    rng = np.random.default_rng(5)
    g = rng.uniform(0.0, 2.0, 500)
    g[::7] = -1.0   # excluded pixels
    g[3::11] = 0.0  # dark pixels
    g[5::13] = 1e-9  # pixels the noise floor pushes below zero half of the time
    out = philox.perturb(g, 0.25, 9, 0.05, 0.01, 0.02, seed=11)
    assert out.shape == (10, 500) and out.dtype == np.float64
    assert np.array_equal(out[0], g)
    neg = g < 0
    assert np.array_equal(out[1:, neg], np.broadcast_to(g[neg], (9, int(neg.sum()))))
    assert np.all(out[1:, ~neg] >= 0.0)
    assert np.any(out[1:, ~neg] == 0.0)  # the clamp is active on this frame
    assert not np.array_equal(out[1], out[2]) and np.all(out[1:, g > 0.5] != g[g > 0.5])
    # pixel0 shifts the global index; one noise term at a time has its own sigma
    half = philox.perturb(g[250:], 0.25, 9, 0.05, 0.01, 0.02, seed=11, pixel0=250)
    assert np.array_equal(half, out[:, 250:])
    z = philox.noise_normals(11, 0.25, np.arange(500, dtype=np.uint64), 1)
    pos = g > 0.5
    for kw, sigma in (({"abs": 0.05}, np.full(500, 0.05)), ({"shot": 0.01}, np.sqrt(0.01 * np.abs(g))),
                      ({"rel": 0.02}, 0.02 * np.abs(g))):
        args = {"abs": 0.0, "shot": 0.0, "rel": 0.0, **kw}
        one = philox.perturb(g, 0.25, 1, seed=11, **args)[1]
        np.testing.assert_allclose(one[pos], (g + sigma * z)[pos], rtol=1e-15, atol=0)
