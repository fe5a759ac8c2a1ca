"""The hold-out scores: the native rule (csrc/native/holdout.cpp) against its NumPy restatement (utils/holdout.py), bit
for bit, on hand-made sums -- zero denominators, an ineligible entry, exact ties, nothing eligible -- and the fallback
entry of a ladder."""
import numpy as np
import pytest

from mpi_cuda_sartsolver_amd.ops import native
from mpi_cuda_sartsolver_amd.utils import holdout as ho

NAMES = ("cv_error", "cv_relative", "train_error", "cv_error_camera", "eligible")


def _both(sums, ok, fallback=0):
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    cv, rel, train, cam, elig, sel, found = native().holdout_scores(sums, ok, fallback)
    nat = {"cv_error": cv, "cv_relative": rel, "train_error": train, "cv_error_camera": cam, "eligible": elig,
           "selected": sel, "found": found}
    ref = ho.scores(sums, ok, fallback)
    for name in NAMES:
        a, b = np.asarray(nat[name]), np.asarray(ref[name])
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, a, b)  # bit for bit, NaNs included
    assert int(nat["selected"]) == int(ref["selected"]) and int(nat["found"]) == int(ref["found"])
    return nat


def _random_sums(rng, nb, K, ncam):
    s = rng.uniform(0.1, 5.0, (nb, K + 1, ncam, 6))
    s[..., 2] = rng.integers(1, 400, (nb, K + 1, ncam))
    s[..., 5] = rng.integers(1, 400, (nb, K + 1, ncam))
    s[:, 0, :, :3] = 0.0  # column 0 holds nothing out
    return s


def test_hand_made_sums():
    # one weight, K = 2, two cameras: the numbers can be followed by hand
    s = np.zeros((1, 3, 2, 6))
    s[0, 0] = [[0, 0, 0, 2.0, 50.0, 8], [0, 0, 0, 6.0, 30.0, 8]]
    s[0, 1] = [[9.0, 20.0, 4, 1.0, 30.0, 4], [16.0, 10.0, 3, 2.0, 20.0, 5]]
    s[0, 2] = [[3.0, 30.0, 4, 1.5, 20.0, 4], [8.0, 20.0, 5, 2.5, 10.0, 3]]
    r = _both(s, np.ones((1, 3)))
    assert r["cv_error"][0] == np.sqrt(36.0 / 16.0) and r["cv_relative"][0] == np.sqrt(36.0 / 80.0)
    assert r["train_error"][0] == np.sqrt(8.0 / 16.0)
    assert np.array_equal(r["cv_error_camera"][0], np.sqrt(np.array([12.0 / 8.0, 24.0 / 8.0])))
    assert r["eligible"][0] == 1 and r["selected"] == 0 and r["found"] == 1


@pytest.mark.parametrize("nb,K,ncam", [(1, 2, 1), (3, 4, 2), (5, 3, 3), (16, 32, 1)])
def test_random_sums_and_the_argmin(nb, K, ncam):
    rng = np.random.default_rng(nb * 100 + K)
    s = _random_sums(rng, nb, K, ncam)
    r = _both(s, np.ones((nb, K + 1)), fallback=nb - 1)
    assert np.all(r["eligible"] == 1) and r["found"] == 1
    assert r["selected"] == int(np.argmin(r["cv_error"]))
    # the order of the additions: columns outer, cameras inner
    num = cnt = 0.0
    for c in range(1, K + 1):
        for m in range(ncam):
            num, cnt = num + s[0, c, m, 0], cnt + s[0, c, m, 2]
    assert r["cv_error"][0] == np.sqrt(num / cnt)


def test_zero_denominators_give_nan():
    s = _random_sums(np.random.default_rng(1), 3, 2, 2)
    s[0, 1:, :, 2] = 0.0   # nothing held out at all: cv_error NaN, cv_relative still a number
    s[1, 1:, 1, 2] = 0.0   # camera 1 never held out
    s[1, 1:, :, 1] = 0.0   # a dark frame: cv_relative NaN
    s[2, 0, :, 5] = 0.0    # nothing kept in column 0
    r = _both(s, np.ones((3, 3)))
    assert np.isnan(r["cv_error"][0]) and np.isfinite(r["cv_relative"][0]) and np.all(np.isnan(r["cv_error_camera"][0]))
    assert np.isfinite(r["cv_error"][1]) and np.isnan(r["cv_relative"][1])
    assert np.isfinite(r["cv_error_camera"][1, 0]) and np.isnan(r["cv_error_camera"][1, 1])
    assert np.isnan(r["train_error"][2]) and np.isfinite(r["cv_error"][2])
    assert list(r["eligible"]) == [0, 1, 1]  # a NaN cv_error is not eligible; a NaN elsewhere does not matter


def test_nan_and_inf_sums_are_not_eligible():
    s = _random_sums(np.random.default_rng(2), 3, 2, 1)
    s[0, 2, 0, 0] = np.nan
    s[1, 1, 0, 0] = np.inf
    r = _both(s, np.ones((3, 3)))
    assert list(r["eligible"]) == [0, 0, 1] and r["selected"] == 2 and r["found"] == 1


def test_an_ineligible_entry_is_skipped():
    s = _random_sums(np.random.default_rng(3), 4, 3, 2)
    s[2, 1:, :, 0] *= 1e-6  # by far the smallest error ...
    ok = np.ones((4, 4))
    full = _both(s, ok)
    assert full["selected"] == 2
    for c in range(4):      # ... but any of its columns stopped on a non-finite iterate, column 0 included
        bad = ok.copy()
        bad[2, c] = 0
        r = _both(s, bad)
        rest = np.where(np.arange(4) == 2, np.inf, r["cv_error"])
        assert r["eligible"][2] == 0 and r["selected"] == int(np.argmin(rest)) and r["found"] == 1
        assert np.array_equal(r["cv_error"], full["cv_error"])  # the scores themselves are still written


def test_exact_ties_go_to_the_first():
    s = _random_sums(np.random.default_rng(4), 4, 2, 2)
    s[1] = s[3] = s[0]
    s[2, 1:, :, 0] *= 4.0
    r = _both(s, np.ones((4, 3)))
    assert r["cv_error"][0] == r["cv_error"][1] == r["cv_error"][3] and r["selected"] == 0
    ok = np.ones((4, 3))
    ok[0, 1] = 0
    assert _both(s, ok)["selected"] == 1


@pytest.mark.parametrize("fallback", [0, 1, 2])
def test_nothing_eligible_takes_the_fallback(fallback):
    s = _random_sums(np.random.default_rng(5), 3, 2, 2)
    r = _both(s, np.zeros((3, 3)), fallback)
    assert not r["eligible"].any() and r["selected"] == fallback and r["found"] == 0
    s[:, 1:, :, 2] = 0.0
    r = _both(s, np.ones((3, 3)), fallback)
    assert not r["eligible"].any() and r["selected"] == fallback and r["found"] == 0


def test_fallback_is_the_entry_nearest_to_beta():
    betas = [0.0, 1e-3, 1e-2, 1e-1]
    for beta, want in ((0.0, 0), (2e-2, 2), (4e-3, 1), (0.5e-3, 0), (1.0, 3), (0.07, 3)):
        assert native().holdout_fallback(np.array(betas), beta) == want == ho.fallback_index(betas, beta), beta
    assert native().holdout_fallback(np.array([0.02]), 0.5) == 0


def test_shapes_are_checked():
    with pytest.raises(ValueError):
        native().holdout_scores(np.zeros((2, 3, 1, 5)), np.ones((2, 3), dtype=np.uint8), 0)
    with pytest.raises(ValueError):
        native().holdout_scores(np.zeros((2, 3, 1, 6)), np.ones((2, 2), dtype=np.uint8), 0)
    with pytest.raises(ValueError):
        native().holdout_scores(np.zeros((2, 3, 1, 6)), np.ones((2, 3), dtype=np.uint8), 2)
