"""Numpy restatement of U^-1 on a Vecchia fit (cocons_vecchia_unwhiten, cocons_sim_vecchia, cocons_vecchia_schedule) on the
oracle's matrices (test infrastructure, not a test module; the blocks are vecchia_reference's).

For observation i with neighbours j_1 < .. < j_k and the block K = C C' in the order (j_1 .. j_k, i): s = C^-T e_last, the
whitening is y_i = sum_t s_t b_{j_t} + s_last b_i and its inverse the recursion x_i = (w_i - sum_t s_t x_{j_t}) / s_last in
ascending i.  level(i) = 0 for the first n_fixed rows, otherwise 1 + the largest level among the row's neighbours (1 without
neighbours)."""
import numpy as np

import vecchia_reference as VR


def coefficients(S, nn, dtype=np.float64):
    """n x (m + 1) in `dtype`: row i holds s_t at place t < k for its neighbours in ascending order, zeros in the free places
    and s_last at place m"""
    S, nn = np.asarray(S), np.asarray(nn)
    n, m = nn.shape
    long_double = np.dtype(dtype) == np.dtype(np.longdouble)
    out = np.zeros((n, m + 1), dtype=dtype)
    for i in range(n):
        idx = np.append(VR.rows_of(nn, i), i)
        C = VR._factor(S[np.ix_(idx, idx)], long_double).astype(dtype)
        k = idx.size - 1
        s = np.zeros(k + 1, dtype=dtype)
        for j in range(k, -1, -1):                      # C' s = e_last, backwards
            rhs = (1 if j == k else 0) - np.sum(C[j + 1:, j] * s[j + 1:], dtype=dtype)
            s[j] = rhs / C[j, j]
        out[i, :k] = s[:k]
        out[i, m] = s[k]
    return out


def unwhiten(S, nn, W, n_fixed=0, x_fixed=None, long_double=False):
    """x (n x c): rows < n_fixed are x_fixed (n_fixed x c), the rows behind them the recursion over the columns W
    ((n - n_fixed) x c)"""
    dt = np.longdouble if long_double else np.float64
    nn = np.asarray(nn)
    n, m = nn.shape
    W = np.asarray(W, dtype=float).reshape(n - n_fixed, -1)
    coef = coefficients(S, nn, dt)
    x = np.zeros((n, W.shape[1]), dtype=dt)
    if n_fixed:
        x[:n_fixed] = np.asarray(x_fixed, dtype=float).reshape(n_fixed, -1)
    for i in range(n_fixed, n):
        idx = VR.rows_of(nn, i)
        acc = np.array(W[i - n_fixed], dtype=dt)
        for t, j in enumerate(idx):
            acc = acc - coef[i, t] * x[j]
        x[i] = acc / coef[i, m]
    return x


def levels(nn, n_fixed=0):
    """n int32: 0 for the first n_fixed rows, otherwise 1 + max over the row's neighbours' levels (the max of nothing is 0)"""
    nn = np.asarray(nn)
    n = nn.shape[0]
    lv = np.zeros(n, dtype=np.int32)
    for i in range(n_fixed, n):
        idx = VR.rows_of(nn, i)
        lv[i] = 1 + (int(np.max(lv[idx])) if idx.size else 0)
    return lv
