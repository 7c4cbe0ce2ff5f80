"""Numpy restatement of the Vecchia approximation (cocons_neg2loglik_vecchia, cocons_vecchia_whiten, cocons_vecchia_predict) on
the oracle's matrices -- Sigma = cov_rns(theta), C = cov_rns_pred(theta) -- (test infrastructure, not a test module).

For observation i with neighbours j_1 < .. < j_k (1-based indices of earlier rows, 0 = none): K = Sigma[(j.., i), (j.., i)],
K = C C', d_i = C[k, k] and the whitened value of a column b is the last component of C^-1 b[(j.., i)].  For a prediction row:
K = Sigma[nb, nb], c = C[row, nb], stochastic = c' K^-1 resid[nb], quadform = c' K^-1 c.

Two precisions: numpy's Cholesky in double, and a hand-written unblocked factorisation in long double for the report's
error of the reference itself.  (The oracle's Sigma is symmetric with the reference's orientation rule already applied, so
reading a block out of it is reading what the device assembles per block.)"""
import numpy as np


def rows_of(nn, i):
    """0-based ascending neighbours of row i of a 1-based, zero-padded table"""
    v = np.asarray(nn)[i]
    return np.sort(v[v > 0]) - 1


def chol_unblocked(K, dtype):
    """Lower factor by the textbook column loop in `dtype`; ValueError(j) at a pivot that is not positive"""
    A = np.array(K, dtype=dtype)
    k = A.shape[0]
    for j in range(k):
        d = A[j, j] - np.sum(A[j, :j] * A[j, :j], dtype=dtype)
        if not d > 0:
            raise ValueError(j)
        A[j, j] = np.sqrt(d)
        for r in range(j + 1, k):
            A[r, j] = (A[r, j] - np.sum(A[r, :j] * A[j, :j], dtype=dtype)) / A[j, j]
    return np.tril(A)


def solve_lower(C, B, dtype):
    Y = np.array(B, dtype=dtype)
    for r in range(C.shape[0]):
        Y[r] = (Y[r] - C[r, :r] @ Y[:r]) / C[r, r]
    return Y


def _factor(K, long_double):
    if long_double:
        return chol_unblocked(K, np.longdouble)
    return np.linalg.cholesky(K)


def whiten(S, nn, B, long_double=False):
    """(U B as n x c, log d as n) for the columns B (n x c)"""
    dt = np.longdouble if long_double else np.float64
    S = np.asarray(S)
    B = np.asarray(B, dtype=float).reshape(S.shape[0], -1)
    n = S.shape[0]
    Y, logd = np.zeros(B.shape, dtype=dt), np.zeros(n, dtype=dt)
    for i in range(n):
        idx = np.append(rows_of(nn, i), i)
        C = _factor(S[np.ix_(idx, idx)], long_double)
        logd[i] = np.log(C[-1, -1])
        Y[i] = solve_lower(C, B[idx], dt)[-1]
    return Y, logd


def neg2loglik(S, nn, Rz, long_double=False):
    """(value, parts) of cocons_neg2loglik_vecchia for the residual columns Rz (n x r)"""
    Y, logd = whiten(S, nn, Rz, long_double)
    n, r = Y.shape
    parts = np.concatenate([[np.sum(logd)], np.sum(Y * Y, axis=0)])
    value = sum(n * np.log(2 * np.pi) + 2 * parts[0] + parts[1 + k] for k in range(r))
    return value, parts


def neg2loglik_exact(S, Rz):
    """the dense value the approximation approaches: sum_k [n log 2 pi + log|Sigma| + r_k' Sigma^-1 r_k]"""
    L = np.linalg.cholesky(S)
    Y = np.linalg.solve(L, Rz)
    n, r = Y.shape
    return float(r * (n * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(L)))) + np.sum(Y * Y))


def all_predecessors(n):
    """the table that makes the approximation exact: row i names 1 .. i - 1 (n x (n - 1), at least one column)"""
    nn = np.zeros((n, max(n - 1, 1)), dtype=np.int32, order="F")
    for i in range(n):
        nn[i, :i] = np.arange(1, i + 1)
    return nn


def predict(S, Cp, nn_pred, resid, long_double=False):
    """(stochastic, quadform) for the prediction rows: Cp = cov_rns_pred (mp x n), resid = z[:, z_col] - X mean (n)"""
    dt = np.longdouble if long_double else np.float64
    mp = Cp.shape[0]
    st, qf = np.zeros(mp, dtype=dt), np.zeros(mp, dtype=dt)
    for i in range(mp):
        idx = rows_of(nn_pred, i)
        if idx.size == 0:
            continue
        C = _factor(np.asarray(S)[np.ix_(idx, idx)], long_double)
        v = solve_lower(C, np.asarray(Cp)[i, idx], dt)
        w = solve_lower(C, np.asarray(resid)[idx], dt)
        st[i], qf[i] = v @ w, v @ v
    return st, qf


def precision_matrix(S, nn):
    """U'U as a dense matrix (U from the blocks: row i holds the last row of C_i^-1 at the block's columns)"""
    n = S.shape[0]
    U = np.zeros((n, n))
    for i in range(n):
        idx = np.append(rows_of(nn, i), i)
        C = np.linalg.cholesky(np.asarray(S)[np.ix_(idx, idx)])
        U[i, idx] = np.linalg.solve(C, np.eye(idx.size))[-1]
    return U.T @ U, U


def profile_value(S, nn, z, xb):
    """sum_k [n log 2 pi + 2 sum log d + z_k' P z_k], P = Q - Q Xb (Xb' Q Xb)^-1 Xb' Q, Q = U'U as a dense matrix"""
    Q, U = precision_matrix(S, nn)
    n = S.shape[0]
    logdet = np.sum(np.log(1.0 / np.diag(U)))      # d_i = 1 / U[i, i]
    V = Q @ xb
    P = Q - V @ np.linalg.solve(xb.T @ V, V.T)
    return float(sum(n * np.log(2 * np.pi) + 2 * logdet + z[:, k] @ P @ z[:, k] for k in range(z.shape[1])))


def reml_value(S, nn, z, X):
    """sum_k [(n - p) log 2 pi + 2 sum log d + log|X' Q X| + z_k' P z_k] with p = rank X"""
    Q, U = precision_matrix(S, nn)
    n = S.shape[0]
    logdet = np.sum(np.log(1.0 / np.diag(U)))
    V = Q @ X
    W = X.T @ V
    P = Q - V @ np.linalg.solve(W, V.T)
    rank = np.linalg.matrix_rank(X)
    return float(sum((n - rank) * np.log(2 * np.pi) + 2 * logdet + np.linalg.slogdet(W)[1] + z[:, k] @ P @ z[:, k]
                     for k in range(z.shape[1])))
