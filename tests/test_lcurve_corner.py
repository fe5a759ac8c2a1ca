"""The native L-curve corner rule (csrc/native/lcurve.cpp) against a NumPy restatement of its definition: the outputs
are equal, not close -- the rule is a handful of fp64 operations in a stated order."""
import math

import numpy as np
import pytest

from mpi_cuda_sartsolver_amd.models.lcurve import lcurve_corner


def corner_reference(rho, eta, ok, fallback):
    """(selected, found, curvature): signed Menger curvature of (log rho, log eta) at every valid point between its
    nearest valid neighbours, the largest one if > 0 (ties to the smaller index), else the fallback rule."""
    nb = len(rho)
    valid = [i for i in range(nb) if ok[i] and math.isfinite(rho[i]) and math.isfinite(eta[i]) and rho[i] > 0
             and eta[i] > 0]
    p = {i: (math.log(rho[i]), math.log(eta[i])) for i in valid}
    curv = np.full(nb, np.nan)
    for m in range(1, len(valid) - 1):
        a, b, c = p[valid[m - 1]], p[valid[m]], p[valid[m + 1]]
        ab = (b[0] - a[0], b[1] - a[1])
        bc = (c[0] - b[0], c[1] - b[1])
        ac = (c[0] - a[0], c[1] - a[1])
        cross = ab[0] * bc[1] - ab[1] * bc[0]
        lab, lbc, lac = (math.sqrt(v[0] * v[0] + v[1] * v[1]) for v in (ab, bc, ac))
        curv[valid[m]] = 0.0 if (lab == 0 or lbc == 0 or lac == 0) else 2.0 * cross / (lab * lbc * lac)
    best, sel = 0.0, None
    for i in range(nb):
        if not np.isnan(curv[i]) and curv[i] > best:
            best, sel = curv[i], i
    if sel is not None:
        return sel, True, curv
    if not valid:
        return fallback, False, curv
    return min(valid, key=lambda i: (abs(i - fallback), i)), False, curv


def check(rho, eta, ok=None, fallback=0):
    rho, eta = np.asarray(rho, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    ok = np.ones(rho.size, dtype=np.uint8) if ok is None else np.asarray(ok, dtype=np.uint8)
    sel, found, curv = lcurve_corner(rho, eta, ok, fallback)
    rsel, rfound, rcurv = corner_reference(rho, eta, ok, fallback)
    assert (sel, found) == (rsel, rfound)
    assert curv.shape == rcurv.shape and np.array_equal(curv, rcurv, equal_nan=True)
    return sel, found, curv


BETAS = np.logspace(-4, 2, 9)


def test_synthetic_l():
    sel, found, curv = check(1 + BETAS ** 2, 1 / (BETAS + 1e-3), fallback=0)
    assert found and 0 < sel < 8
    assert np.isnan(curv[0]) and np.isnan(curv[-1]) and np.all(np.isfinite(curv[1:-1]))
    assert curv[sel] == np.nanmax(curv) and curv[sel] > 0


@pytest.mark.parametrize("fallback", [0, 3, 8])
def test_straight_line_falls_back(fallback):
    # a horizontal line in log-log: every log eta difference is exactly 0, so every cross product is exactly 0
    sel, found, curv = check(2.0 ** np.arange(9), np.full(9, 3.0), fallback=fallback)
    assert not found and sel == fallback
    assert np.all(curv[1:-1] == 0)
    # a sloped line: the cross products are rounding noise of either sign; only equality with the restatement is asked
    check(2.0 ** np.arange(9), 3.0 ** -np.arange(9), fallback=fallback)


def test_concave_curve_has_no_corner():
    # bending the other way (cross < 0 everywhere): no corner, whatever the magnitude
    sel, found, curv = check(1 / (BETAS + 1e-3), 1 + BETAS ** 2, fallback=2)
    assert not found and sel == 2 and np.all(curv[1:-1] <= 0)


def test_invalid_point_is_bridged():
    rho, eta = 1 + BETAS ** 2, 1 / (BETAS + 1e-3)
    ok = np.ones(9, dtype=np.uint8)
    ok[4] = 0
    sel, found, curv = check(rho, eta, ok)
    assert np.isnan(curv[4]) and np.isfinite(curv[3]) and np.isfinite(curv[5])
    # its neighbours take each other: the same numbers as the curve without the point
    _, _, c8 = check(np.delete(rho, 4), np.delete(eta, 4))
    assert np.array_equal(np.delete(curv, 4), c8, equal_nan=True)
    for bad in (np.nan, np.inf, 0.0, -1.0):  # a norm that is not finite and > 0 drops the point in the same way
        r2 = rho.copy()
        r2[4] = bad
        _, _, c2 = check(r2, eta)
        assert np.array_equal(c2, curv, equal_nan=True)
        e2 = eta.copy()
        e2[4] = bad
        _, _, c3 = check(rho, e2)
        assert np.array_equal(c3, curv, equal_nan=True)


def test_coincident_points_give_zero():
    rho, eta = 1 + BETAS ** 2, 1 / (BETAS + 1e-3)
    rho[3], eta[3] = rho[2], eta[2]
    _, _, curv = check(rho, eta)
    assert curv[2] == 0 and curv[3] == 0


@pytest.mark.parametrize("fallback", [0, 5])
def test_all_invalid(fallback):
    sel, found, curv = check(1 + BETAS ** 2, 1 / (BETAS + 1e-3), np.zeros(9, dtype=np.uint8), fallback)
    assert not found and sel == fallback and np.all(np.isnan(curv))


def test_fallback_moves_to_the_nearest_valid_point():
    rho, eta = 2.0 ** np.arange(7), np.full(7, 3.0)  # a horizontal line: no corner
    ok = np.array([1, 1, 0, 0, 0, 1, 1], dtype=np.uint8)
    assert check(rho, eta, ok, fallback=2)[0] == 1
    assert check(rho, eta, ok, fallback=4)[0] == 5
    assert check(rho, eta, ok, fallback=3)[0] == 1  # a tie goes to the smaller index


def test_ties_go_to_the_smaller_index():
    # down, right, up: the two right angles have the same side lengths (u, v) in either order, so their curvatures are
    # the same products of the same numbers
    sel, found, curv = check([1.0, 1.0, 2.0, 2.0], [4.0, 1.0, 1.0, 4.0])
    assert found and curv[1] == curv[2] and curv[1] > 0 and sel == 1


def test_fewer_than_three_valid_points():
    sel, found, curv = check([1.0, 2.0, 3.0], [3.0, 2.0, 1.0], [1, 0, 1], fallback=1)
    assert not found and sel == 0 and np.all(np.isnan(curv))
