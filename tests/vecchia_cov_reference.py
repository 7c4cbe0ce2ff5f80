"""Numpy restatement of U^-T on a Vecchia fit (cocons_vecchia_unwhiten_t, cocons_vecchia_cov_mult, cocons_vecchia_cov_cols,
cocons_vecchia_schedule_t) on vecchia_sim_reference.coefficients (test infrastructure, not a test module).

With U(i, j_t) = s_t and U(i, i) = s_last(i), and U_pp the block of U on the rows and columns >= n_fixed: v = U_pp^-T w is the
recursion in descending j = n - 1 .. n_fixed, v_j = (w_j - sum_{k names j} U(k, j) v_k) / s_last(j), the sum over ascending k.
tlevel(j) = 0 for j < n_fixed, otherwise 1 + the largest tlevel among the rows that name j (1 when nobody does).
cov_mult = U_pp^-1 U_pp^-T: the descending recursion, then vecchia_sim_reference's ascending one with the fixed rows at zero.

The restatement in double against itself in long double (tests/test_vecchia_cov_reference.py prints the figures; relative to
the largest magnitude, oracle's matrices at n = 40): unwhiten_t 2.4e-16 (m = 5), 1.4e-16 (m = 5, n_fixed = 13) and 2.2e-16
(m = 39, n_fixed = 24); cov_mult 1.9e-16, 4.7e-16 and 3.1e-16 on the same cases -- seven orders below the PARITY bound of 1e-8
the tests hold the device to."""
import numpy as np

import vecchia_reference as VR
import vecchia_sim_reference as VS


def named_by(nn):
    """per column j the (row k, place t) pairs with U(k, j) = coef[k, t], ascending in k"""
    nn = np.asarray(nn)
    out = [[] for _ in range(nn.shape[0])]
    for k in range(nn.shape[0]):
        for t, j in enumerate(VR.rows_of(nn, k)):
            out[j].append((k, t))
    return out


def dense_u(coef, nn):
    """U as a dense n x n matrix in the coefficients' type"""
    nn = np.asarray(nn)
    n, m = nn.shape
    U = np.zeros((n, n), dtype=coef.dtype)
    for i in range(n):
        idx = VR.rows_of(nn, i)
        U[i, idx] = coef[i, :idx.size]
        U[i, i] = coef[i, m]
    return U


def solve_t(coef, nn, W, n_fixed=0):
    """v ((n - n_fixed) x c) = U_pp^-T W in the coefficients' type"""
    nn = np.asarray(nn)
    n, m = nn.shape
    dt = coef.dtype
    W = np.asarray(W, dtype=float).reshape(n - n_fixed, -1)
    lists = named_by(nn)
    v = np.zeros((n, W.shape[1]), dtype=dt)
    for j in range(n - 1, n_fixed - 1, -1):
        acc = np.zeros(W.shape[1], dtype=dt)
        for k, t in lists[j]:
            acc = acc + coef[k, t] * v[k]
        v[j] = (np.array(W[j - n_fixed], dtype=dt) - acc) / coef[j, m]
    return v[n_fixed:]


def solve(coef, nn, W, n_fixed=0):
    """x ((n - n_fixed) x c) = U_pp^-1 W: vecchia_sim_reference.unwhiten's recursion with the fixed rows at zero"""
    nn = np.asarray(nn)
    n, m = nn.shape
    dt = coef.dtype
    W = np.asarray(W).reshape(n - n_fixed, -1)
    x = np.zeros((n, W.shape[1]), dtype=dt)
    for i in range(n_fixed, n):
        acc = np.array(W[i - n_fixed], dtype=dt)
        for t, j in enumerate(VR.rows_of(nn, i)):
            acc = acc - coef[i, t] * x[j]
        x[i] = acc / coef[i, m]
    return x[n_fixed:]


def _dtype(long_double):
    return np.longdouble if long_double else np.float64


def unwhiten_t(S, nn, W, n_fixed=0, long_double=False, coef=None):
    coef = VS.coefficients(S, nn, _dtype(long_double)) if coef is None else coef
    return solve_t(coef, nn, W, n_fixed)


def cov_mult(S, nn, B, n_fixed=0, long_double=False, coef=None):
    coef = VS.coefficients(S, nn, _dtype(long_double)) if coef is None else coef
    return solve(coef, nn, solve_t(coef, nn, B, n_fixed), n_fixed)


def tlevels(nn, n_fixed=0):
    """n int32: 0 for the first n_fixed rows, otherwise 1 + max over the tlevels of the rows that name the row"""
    nn = np.asarray(nn)
    n = nn.shape[0]
    lists = named_by(nn)
    lv = np.zeros(n, dtype=np.int32)
    for j in range(n - 1, n_fixed - 1, -1):
        lv[j] = 1 + max((int(lv[k]) for k, _ in lists[j]), default=0)
    return lv
