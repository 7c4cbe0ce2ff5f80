"""Numpy statement of the analytic gradient of the Vecchia -2 log-likelihood (cocons_neg2loglik_grad_vecchia; test
infrastructure, not a test module).

For observation i the block is C = L L' (the neighbours, then the observation), w_c = L^-1 b_c, y_c its last component,
s = L^-T e_last and h = L^-T v with v = sum_c y_c (w_c with its last component set to 0).  The block's term
f_i = c 2 log d_i + sum_c y_c^2 has the derivative <W_i, dC> with

    W_log = c s s',      W_quad = -(sum_c y_c^2) s s' - (h s' + s h').

The n x n weight matrix W = sum_i scatter(W_i) is contracted with the pair partials of the dense gradient's statement
(grad_reference.py: site_quantities, matern_and_partials, select_mode), and df_i/db_c = 2 y_c s gives the mean gradient."""
from __future__ import annotations

import math

import numpy as np

from grad_reference import EPS, matern_and_partials, select_mode, site_quantities
from vecchia_reference import rows_of


def block_weights(S, nn, B):
    """(W_log, W_quad, gb, Y, logd): the two n x n weight matrices, gb[i, c] = df/dB[i, c], the whitened columns and log d"""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    c = B.shape[1]
    Wl, Wq, gb = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, c))
    Y, logd = np.zeros((n, c)), np.zeros(n)
    for i in range(n):
        idx = np.append(rows_of(nn, i), i)
        L = np.linalg.cholesky(S[np.ix_(idx, idx)])
        w = np.linalg.solve(L, B[idx])
        y = w[-1].copy()
        e = np.zeros(idx.size)
        e[-1] = 1.0
        s = np.linalg.solve(L.T, e)
        w0 = w.copy()
        w0[-1] = 0.0
        h = np.linalg.solve(L.T, w0 @ y)
        ss = np.outer(s, s)
        Wl[np.ix_(idx, idx)] += c * ss
        Wq[np.ix_(idx, idx)] += -(y @ y) * ss - (np.outer(h, s) + np.outer(s, h))
        gb[idx] += 2.0 * np.outer(s, y)
        Y[i], logd[i] = y, math.log(L[-1, -1])
    return Wl, Wq, gb, Y, logd


def sigma_and_contract(T, locs, X, smooth_limits, weights):
    """(Sigma, [6 x p table for every symmetric n x n weight matrix W in `weights`]): sum_ij W_ij dSigma_ij / dtheta in the
    conventions of cocons_neg2loglik_grad_dense (scale[0] takes the global-range sum, scale[k >= 1] the factor 2)"""
    T = np.asarray(T, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    n, p = X.shape
    mode, nu_fixed, smooth_free = select_mode(T, smooth_limits)
    gr = math.exp(2 * T[1, 0])
    st = site_quantities(T, X, smooth_limits)
    jj, ii = np.tril_indices(n, -1)                # ii < jj: the first ("ii") location is the lower index
    rd, a, t = st["rd"], st["a"], st["t"]
    ra, ct, sn = rd * a, np.cos(t), np.sin(t)
    s11 = (rd[ii] + rd[jj]) / 2
    s22 = (rd[ii] * a[ii] ** 2 + rd[jj] * a[jj] ** 2) / 2
    s12 = (ra[ii] * ct[ii] + ra[jj] * ct[jj]) / 2
    D = s11 * s22 - s12 ** 2
    dx = locs[ii, 0] - locs[jj, 0]
    dy = locs[ii, 1] - locs[jj, 1]
    q = s22 * dx * dx + s11 * dy * dy - 2 * s12 * dx * dy
    if mode.startswith("geom"):                    # (a fixed smoothness outside the closed forms: every site has nu = lo)
        nu = np.sqrt(st["nu"][ii]) * np.sqrt(st["nu"][jj])
    else:
        nu = np.full_like(q, nu_fixed)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.sqrt(8 * nu * q / (gr * D))
    coinc = u <= EPS
    far = u >= 706
    live = ~coinc & ~far
    M, Mu, Mn = np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    M[live], Mu[live], Mn[live] = matern_and_partials(nu[live], u[live], "geom" if mode.startswith("geom") else mode)
    if not smooth_free:
        Mn[:] = 0
    P = st["sigma"][ii] * st["sigma"][jj] * np.sqrt(ra[ii] * sn[ii] * ra[jj] * sn[jj] / D)
    C = M * P
    diag = st["sd"] + st["ng"]
    Sigma = np.diag(diag)
    off = np.where(coinc, diag[ii], C)
    Sigma[ii, jj] = off
    Sigma[jj, ii] = off
    with np.errstate(divide="ignore", invalid="ignore"):
        U = np.where(live, P * Mu * u, 0.0)
        Cl = np.where(live, C, 0.0)
    # the partials per pair and side, once; every weight matrix is contracted with the same numbers
    per_side = []
    for side in (ii, jj):
        rdi, ai, rai, cti, sni, tpi = rd[side], a[side], ra[side], ct[side], sn[side], st["tp"][side]
        fams = (
            (1, rdi / 2, rdi * ai ** 2 / 2, rai * cti / 2, 0.5),
            (2, 0.0, rdi * ai ** 2, rai * cti / 2, 0.5),
            (3, 0.0, 0.0, -rai * sni * tpi / 2, 0.5 * cti / sni * tpi),
        )
        d = {}
        for fam, s11p, s22p, s12p, amp in fams:
            Dp = s11p * s22 + s11 * s22p - 2 * s12 * s12p
            qp = s22p * dx * dx + s11p * dy * dy - 2 * s12p * dx * dy
            with np.errstate(divide="ignore", invalid="ignore"):
                v = U * 0.5 * (qp / q - Dp / D) + Cl * (amp - 0.5 * Dp / D)
            d[fam] = np.where(live, v, 0.0)
        d[0] = 0.5 * Cl
        if smooth_free:
            dl = st["dnu"][side] / (2 * st["nu"][side])
            d[4] = np.where(live, P * Mn * nu * dl + U * 0.5 * dl, 0.0)
        per_side.append((side, d))
    tables = []
    for W in weights:
        W = np.asarray(W, dtype=np.float64)
        w2 = 2 * W[ii, jj]
        g = np.zeros((6, n))
        for side, d in per_side:
            for fam, v in d.items():
                g[fam] += np.bincount(side, w2 * v, minlength=n)
        g[0] += np.bincount(ii, np.where(coinc, w2 * st["sd"][ii], 0.0), minlength=n)     # coincident: the ii site's diagonal
        g[5] += np.bincount(ii, np.where(coinc, w2 * st["ng"][ii], 0.0), minlength=n)
        dW = np.diag(W)
        g[0] += dW * st["sd"]
        g[5] += dW * st["ng"]
        gt = (X.T @ g.T).T.copy()
        gt[1, 1:] *= 2
        gt[1, 0] = float(np.sum(w2 * -U))
        tables.append(gt)
    return Sigma, tables


def neg2loglik_grad(T, mean, locs, X, z, smooth_limits, nn, B=None, Sigma=None):
    """(value, parts, grad_table, grad_quad, grad_mean) of cocons_neg2loglik_grad_vecchia; with B (n x c) the columns are
    used as given and grad_mean is None.  Sigma: the matrix the blocks are read from (default: this statement's own, which
    the tests hold against the oracle's)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    own, _ = sigma_and_contract(T, locs, X, smooth_limits, [])
    S = own if Sigma is None else np.asarray(Sigma, dtype=np.float64)
    if B is None:
        cols = np.asarray(z, dtype=np.float64).reshape(n, -1) - (X @ np.asarray(mean, dtype=np.float64))[:, None]
    else:
        cols = np.asarray(B, dtype=np.float64).reshape(n, -1)
    Wl, Wq, gb, Y, logd = block_weights(S, nn, cols)
    _, (gl, gq) = sigma_and_contract(T, locs, X, smooth_limits, [Wl, Wq])
    parts = np.concatenate([[np.sum(logd)], np.sum(Y * Y, axis=0)])
    value = float(sum(n * math.log(2 * math.pi) + 2 * parts[0] + parts[1 + k] for k in range(cols.shape[1])))
    gm = None if B is not None else -(X.T @ gb.sum(axis=1))
    return value, parts, gl + gq, gq, gm


def _gls(S, nn, z, xb):
    """(U, W = xb' U'U xb, beta, the residual columns z - xb beta) for the approximation's U"""
    from vecchia_reference import precision_matrix
    Q, U = precision_matrix(S, nn)
    W = xb.T @ Q @ xb
    beta = np.linalg.solve(W, xb.T @ Q @ z)
    return U, W, beta, z - xb @ beta


def profile_grad(T, locs, X, z, xb, smooth_limits, nn):
    """(value, 6 x p table) of the profiled value (vecchia_reference.profile_value): by the envelope theorem the gradient at
    fixed beta-hat, i.e. the entry's with B = z_k - xb beta_k"""
    n = np.asarray(X).shape[0]
    z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    xb = np.asarray(xb, dtype=np.float64).reshape(n, -1)
    S, _ = sigma_and_contract(T, locs, X, smooth_limits, [])
    _, _, _, E = _gls(S, nn, z, xb)
    val, _, gt, _, _ = neg2loglik_grad(T, None, locs, X, None, smooth_limits, nn, B=E)
    return val, gt


def reml_grad(T, locs, X, z, smooth_limits, nn):
    """(value, 6 x p table) of vecchia_reference.reml_value: B = [residual columns | sqrt(r) V], V = X chol(X' U'U X)^-T, the
    log-determinant's share scaled to r realisations, the quadratic forms' share as it is"""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    r = z.shape[1]
    S, _ = sigma_and_contract(T, locs, X, smooth_limits, [])
    _, W, _, E = _gls(S, nn, z, X)
    Lw = np.linalg.cholesky(W)
    V = np.linalg.solve(Lw, X.T).T
    B = np.hstack([E, math.sqrt(r) * V])
    _, parts, gt, gq, _ = neg2loglik_grad(T, None, locs, X, None, smooth_limits, nn, B=B)
    rank = int(np.linalg.matrix_rank(X))
    val = float(sum((n - rank) * math.log(2 * math.pi) + 2 * parts[0] + 2 * np.sum(np.log(np.diag(Lw))) + parts[1 + k]
                    for k in range(r)))
    return val, (gt - gq) * (r / B.shape[1]) + gq
