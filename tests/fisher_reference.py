"""Independent numpy / scipy statement of the expected (Fisher) information of the dense model (test infrastructure).

Sigma = cov_rns(theta) in the caller's order and the 6 p dense matrices dSigma / dtheta[t, k], from the closed form of every
entry (grad_reference.site_quantities, matern_and_partials) under the conventions of the gradient's table: scale k = 0 is
the global range, scale k >= 1 enters the site predictor with the factor 2, a coincident pair (u <= eps) takes the first
site's diagonal, u >= 706 contributes 0.  Then I[a, b] = (r / 2) tr(Sigma^-1 Sigma_a Sigma^-1 Sigma_b) in two forms.
"""
from __future__ import annotations

import math

import numpy as np
from scipy import linalg

import grad_reference as GR

EPS = GR.EPS


def _pairs(T, locs, X, smooth_limits):
    """Sigma and, per pair ii < jj, the partials with respect to the site predictors of both sides (6 x npairs each) and to
    the global range; the site quantities."""
    T = np.asarray(T, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    n, p = X.shape
    mode, nu_fixed, smooth_free = GR.select_mode(T, smooth_limits)
    gr = math.exp(2 * T[1, 0])
    st = GR.site_quantities(T, X, smooth_limits)
    ii, jj = np.tril_indices(n, -1)
    ii, jj = jj, ii                                # ii < jj
    rd, a, t = st["rd"], st["a"], st["t"]
    ra, ct, sn = rd * a, np.cos(t), np.sin(t)
    s11 = (rd[ii] + rd[jj]) / 2
    s22 = (rd[ii] * a[ii] ** 2 + rd[jj] * a[jj] ** 2) / 2
    s12 = (ra[ii] * ct[ii] + ra[jj] * ct[jj]) / 2
    D = s11 * s22 - s12 ** 2
    dx = locs[ii, 0] - locs[jj, 0]
    dy = locs[ii, 1] - locs[jj, 1]
    q = s22 * dx * dx + s11 * dy * dy - 2 * s12 * dx * dy
    if mode in ("geom", "geom0"):
        nu = np.sqrt(st["nu"][ii]) * np.sqrt(st["nu"][jj]) if mode == "geom" else np.zeros_like(q)
    else:
        nu = np.full_like(q, nu_fixed)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.sqrt(8 * nu * q / (gr * D))
    coinc = u <= EPS
    live = ~coinc & ~(u >= 706)
    M, Mu, Mn = np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    M[live], Mu[live], Mn[live] = GR.matern_and_partials(nu[live], u[live], "geom" if mode.startswith("geom") else mode)
    if not smooth_free:
        Mn[:] = 0
    P = st["sigma"][ii] * st["sigma"][jj] * np.sqrt(ra[ii] * sn[ii] * ra[jj] * sn[jj] / D)
    C = np.where(live, M * P, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        U = np.where(live, P * Mu * u, 0.0)
    diag = st["sd"] + st["ng"]
    Sigma = np.diag(diag)
    off = np.where(coinc, diag[ii], C)
    Sigma[ii, jj] = off
    Sigma[jj, ii] = off
    # per pair and side: the partial with respect to the site predictor of every family (6 x npairs)
    d_side = []
    for side in (ii, jj):
        rdi, ai, rai, cti, sni, tpi = rd[side], a[side], ra[side], ct[side], sn[side], st["tp"][side]
        d = np.zeros((6, u.size))
        parts = (
            (1, rdi / 2, rdi * ai ** 2 / 2, rai * cti / 2, 0.5),
            (2, 0.0, rdi * ai ** 2, rai * cti / 2, 0.5),
            (3, 0.0, 0.0, -rai * sni * tpi / 2, 0.5 * cti / sni * tpi),
        )
        for fam, s11p, s22p, s12p, amp in parts:
            Dp = s11p * s22 + s11 * s22p - 2 * s12 * s12p
            qp = s22p * dx * dx + s11p * dy * dy - 2 * s12p * dx * dy
            with np.errstate(divide="ignore", invalid="ignore"):
                v = U * 0.5 * (qp / q - Dp / D) + C * (amp - 0.5 * Dp / D)
            d[fam] = np.where(live, v, 0.0)
        d[0] = 0.5 * C
        if smooth_free:
            dl = st["dnu"][side] / (2 * st["nu"][side])
            d[4] = np.where(live, P * Mn * nu * dl + U * 0.5 * dl, 0.0)
        d_side.append(d)
    # coincident pairs: the ii site's diagonal value, a function of the ii site's std.dev and nugget predictors alone
    d_side[0][0] += np.where(coinc, st["sd"][ii], 0.0)
    d_side[0][5] += np.where(coinc, st["ng"][ii], 0.0)
    return Sigma, ii, jj, d_side, -U, st                # (the global range: gr = e^(2 theta), dlog u = -1)


def sigma_and_partials(T, locs, X, smooth_limits):
    """(Sigma n x n, dS 6 x p x n x n) in float64; T the 6 x p table."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    Sigma, ii, jj, d_side, dglob, st = _pairs(T, locs, X, smooth_limits)
    dS = np.zeros((6, p, n, n))
    idx = np.arange(n)
    for f in range(6):
        for k in range(p):
            if f == 1 and k == 0:
                e = dglob
            else:
                c = 2.0 if f == 1 else 1.0
                e = c * (d_side[0][f] * X[ii, k] + d_side[1][f] * X[jj, k])
            dS[f, k][ii, jj] = e
            dS[f, k][jj, ii] = e
            if f == 0:
                dS[f, k][idx, idx] = st["sd"] * X[:, k]
            elif f == 5:
                dS[f, k][idx, idx] = st["ng"] * X[:, k]
    return Sigma, dS


def sigma_and_directions(T, locs, X, smooth_limits, dirs):
    """(Sigma, Sigma_a for the ndir x 6 x p directions) without the 6 p dense matrices: the directions' site weights
    w_a[f] = c_f X v_a[f] (c = 2 for scale, whose k = 0 is the global range) applied pair by pair."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    Sigma, ii, jj, d_side, dglob, st = _pairs(T, locs, X, smooth_limits)
    V = np.asarray(dirs, dtype=np.float64).reshape(-1, 6, p)
    Sa = np.zeros((V.shape[0], n, n))
    idx = np.arange(n)
    for a, v in enumerate(V):
        w = X @ v.T                                 # n x 6
        w[:, 1] = 2 * (X[:, 1:] @ v[1, 1:])
        e = dglob * v[1, 0]
        for f in range(6):
            e = e + d_side[0][f] * w[ii, f] + d_side[1][f] * w[jj, f]
        Sa[a][ii, jj] = e
        Sa[a][jj, ii] = e
        Sa[a][idx, idx] = st["sd"] * w[:, 0] + st["ng"] * w[:, 5]
    return Sigma, Sa


def direction_matrices(dS, dirs):
    """Sigma_a = sum_tk dirs[a][t, k] dS[t, k] for ndir x 6 x p (or ndir x 6p) directions."""
    six, p, n, _ = dS.shape
    V = np.asarray(dirs, dtype=np.float64).reshape(-1, six * p)
    return np.tensordot(V, dS.reshape(six * p, n, n), axes=1)


def info_solve(Sigma, Sa, r=1):
    """(r / 2) sum G_a o G_b' with G_a = Sigma^-1 Sigma_a by cho_solve."""
    cf = linalg.cho_factor(Sigma, lower=True)
    G = np.stack([linalg.cho_solve(cf, S) for S in Sa])
    nd = G.shape[0]
    return 0.5 * r * (G.reshape(nd, -1) @ np.ascontiguousarray(G.transpose(0, 2, 1)).reshape(nd, -1).T)


def info_whiten(Sigma, Sa, r=1):
    """(r / 2) <L^-1 Sigma_a L^-T, L^-1 Sigma_b L^-T>."""
    L = linalg.cholesky(Sigma, lower=True)
    Ms = []
    for S in Sa:
        Y = linalg.solve_triangular(L, S, lower=True)
        Ms.append(linalg.solve_triangular(L, Y.T, lower=True))
    Ms = np.stack(Ms)
    nd = Ms.shape[0]
    return 0.5 * r * (Ms.reshape(nd, -1) @ Ms.reshape(nd, -1).T)


def metric(I, R):
    """max_ab |I_ab - R_ab| / sqrt(R_aa R_bb), zero diagonals replaced by 1."""
    d = np.sqrt(np.where(np.diag(R) == 0, 1.0, np.diag(R)))
    return float(np.max(np.abs(np.asarray(I) - R) / np.outer(d, d)))


def scaling_direction(p):
    """v_s = e_{sd,0} + e_{ng,0}: Sigma(sd0 + d, ng0 + d) = e^d Sigma, so Sigma_v = Sigma and I(v_s, v_s) = r n / 2."""
    v = np.zeros((6, p))
    v[0, 0] = 1.0
    v[5, 0] = 1.0
    return v
