"""Reference and error bound shared by the roughness tests (not a test module), derived as tests/fit_bound.py derives
its own.

A row's sum s_r = sum_k L_rk u_k of m_r terms, fused or not and in any order, is within gamma_{m_r} a_r of the exact
value, a_r = sum_k |L_rk| |u_k| (gamma_n ~ n 2^-53), so its square is within 2 gamma a_r^2 (+ one rounding) of the
exact square, and a sum of n squares adds gamma_n sum a_r^2. NumPy's reference carries the same bounds, so

    |eta2 - eta2_ref| <= 4 (n + m + 4) 2^-53 sum_r a_r^2,    m the longest row.

In log mode u = log(max(x, 1e-100)) comes from two correctly-rounded-to-an-ulp-or-two logarithms (the device's and
NumPy's): a relative 4 2^-53 on every |u_k|, i.e. 8 2^-53 a_r^2 per row -- inside the n term's slack for every n used.
"""
import numpy as np

U = 2.0 ** -53


def reference(row_ptr, col, val, X, log=False):
    """(eta2_ref [nv], bound [nv]) for X [nv, >= n]: entries at and beyond n = len(row_ptr) - 1 are not read."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = row_ptr.size - 1
    col = np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)  # widening fp32 is exact
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))[:, :n]
    Uv = np.log(np.maximum(X, 1e-100)) if log else X
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    m = int(np.diff(row_ptr).max()) if n else 0
    eta2, bound = np.zeros(X.shape[0]), np.zeros(X.shape[0])
    for j in range(X.shape[0]):
        s, a = np.zeros(n), np.zeros(n)
        np.add.at(s, rows, val * Uv[j, col])
        np.add.at(a, rows, np.abs(val) * np.abs(Uv[j, col]))
        eta2[j] = np.sum(s * s)
        bound[j] = 4.0 * (n + m + 4) * U * np.sum(a * a)
    return eta2, bound
