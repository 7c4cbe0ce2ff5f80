"""Numpy statement of the grouped Vecchia gradient (cocons_neg2loglik_grad_vecchia_grouped; test
infrastructure, not a test module).

A block has the rows S ascending, the member set M, C = L L', Z = L^-1 and w_c = Z b_c.  It contributes
f = sum_{p in M} (nb 2 log L_pp + sum_c w_c[p]^2), whose derivative is <W, dC> with W = Z' P Z, N = sum_c w_c w_c',

    P_log  = nb diag([p in M]),
    P_quad: P_pp = -[p in M] N_pp,   P_pj = P_jp = -[p in M] N_pj for j < p,

and df/db_c = 2 Z' ([p in M] w_c).  W is built per block from the plan of group_reference.plan -- by the two triangular
products, not by the members' solves the kernel runs -- and contracted as vecchia_grad_reference contracts."""
from __future__ import annotations

import math

import numpy as np

import group_reference as GRP
from vecchia_grad_reference import sigma_and_contract


def block_weights(S, pl, B):
    """(W_log, W_quad, gb, Y, logd) over the blocks of the plan `pl`: the two n x n weight matrices, gb[i, c] = df/dB[i, c],
    the members' whitened values and log d"""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    nb = B.shape[1]
    Wl, Wq, gb = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, nb))
    Y, logd = np.zeros((n, nb)), np.zeros(n)
    for b in range(pl["blocks"]):
        idx = np.asarray(pl["rows"][pl["off"][b]:pl["off"][b + 1]], dtype=np.int64)
        k = idx.size
        mem = np.array([(int(pl["mask"][b]) >> q) & 1 for q in range(k)], dtype=np.float64)
        L = np.linalg.cholesky(S[np.ix_(idx, idx)])
        Z = np.linalg.solve(L, np.eye(k))
        w = Z @ B[idx]
        N = w @ w.T
        low = np.tril(N, -1) * mem[:, None]                 # row p of a member: N[p, j], j < p
        Pq = -(np.diag(np.diag(N) * mem) + low + low.T)
        Wl[np.ix_(idx, idx)] += nb * (Z.T @ (mem[:, None] * Z))
        Wq[np.ix_(idx, idx)] += Z.T @ Pq @ Z
        gb[idx] += 2.0 * (Z.T @ (mem[:, None] * w))
        on = mem > 0
        Y[idx[on]] = w[on]
        logd[idx[on]] = np.log(np.diag(L))[on]
    return Wl, Wq, gb, Y, logd


def neg2loglik_grad(T, mean, locs, X, z, smooth_limits, nn, group, B=None, Sigma=None):
    """(value, parts, grad_table, grad_quad, grad_mean) of cocons_neg2loglik_grad_vecchia_grouped for the partition `group`
    of the table `nn` (the caller's, or the expanded one: both have the same plan); with B (n x c) the columns are used as
    given and grad_mean is None"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    own, _ = sigma_and_contract(T, locs, X, smooth_limits, [])
    S = own if Sigma is None else np.asarray(Sigma, dtype=np.float64)
    if B is None:
        cols = np.asarray(z, dtype=np.float64).reshape(n, -1) - (X @ np.asarray(mean, dtype=np.float64))[:, None]
    else:
        cols = np.asarray(B, dtype=np.float64).reshape(n, -1)
    Wl, Wq, gb, Y, logd = block_weights(S, GRP.plan(nn, group), cols)
    _, (gl, gq) = sigma_and_contract(T, locs, X, smooth_limits, [Wl, Wq])
    parts = np.concatenate([[np.sum(logd)], np.sum(Y * Y, axis=0)])
    value = float(sum(n * math.log(2 * math.pi) + 2 * parts[0] + parts[1 + k] for k in range(cols.shape[1])))
    gm = None if B is not None else -(X.T @ gb.sum(axis=1))
    return value, parts, gl + gq, gq, gm
