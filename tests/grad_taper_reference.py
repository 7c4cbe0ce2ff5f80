"""Independent numpy / scipy statement of the analytic gradient of the tapered -2 log-likelihood (test infrastructure).

S = T o C(theta) on a symmetric CSR pattern (1-based, diagonal stored), C = cov_rns_taper: isotropic, per site
sigma_i^2 = exp(x_i' theta_sd), rho_i = exp(2 x_i' theta_scale) (the FULL scale vector), nu_i by the logistic link,
g_i = exp(x_i' theta_nugget); for i != j  nu = sqrt(nu_i nu_j), u = sqrt(8 nu) h / sqrt((rho_i + rho_j) / 2),
P = 2 sqrt(rho_i rho_j) / (rho_i + rho_j) sigma_i sigma_j, C = P M_nu(u); the diagonal is sigma_i^2 + g_i.

f = sum_k [ n log 2 pi + log det S + R_k' S^-1 R_k ],  R = Z - X mean, A = S^-1 R:
    d f / d theta_a = sum over the pattern of W_ij T_ij dC_ij / d theta_a,   W = r S^-1 - A A',   d f / d mean = -2 X' A 1.
The two terms of W -- log-determinant part and quadratic-form part -- are returned apart.  S^-1 is the dense inverse of the
assembled matrix; the Matern part uses scipy.special.kv / kvp and a Richardson difference in nu (grad_reference.py).

Also here: the selected inverse on a tile envelope in numpy (the recursion the library runs on 128 x 128 tiles).
"""
from __future__ import annotations

import os
import sys

import numpy as np
from scipy import linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grad_reference import EPS, matern_and_partials, select_mode  # noqa: E402


def wendland1_pattern(locs, delta):
    """(colindices, rowpointers, entries) of the Wendland-1 taper (1 - h)^4 (4 h + 1), h = d / delta < 1: 1-based CSR."""
    locs = np.asarray(locs, dtype=np.float64)
    n = locs.shape[0]
    d = np.sqrt(((locs[:, None, :] - locs[None, :, :]) ** 2).sum(axis=2))
    ci, rp, ent = [], [1], []
    for i in range(n):
        js = np.nonzero(d[i] < delta)[0]
        h = d[i, js] / delta
        ci.extend((js + 1).tolist())
        ent.extend(((1 - h) ** 4 * (4 * h + 1)).tolist())
        rp.append(len(ci) + 1)
    return np.asarray(ci, dtype=np.int32), np.asarray(rp, dtype=np.int32), np.asarray(ent)


def taper_matrix(T, locs, X, smooth_limits, ref_taper):
    """The dense S = T o C(theta) as the library assembles it (a coincident pair takes the diagonal value of the site with
    the larger index: the row site of the lower triangle) and everything the gradient needs per stored entry."""
    T = np.asarray(T, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    n = X.shape[0]
    ci, rp, te = ref_taper
    ci = np.asarray(ci, dtype=np.int64)
    rp = np.asarray(rp, dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    cols = ci - 1
    lo, hi = smooth_limits
    mode, nu_fixed, smooth_free = select_mode(T, smooth_limits)
    # n x 6: sd, scale, aniso, tilt, smooth, nugget (intercepts added apart: a -Inf nugget intercept stays -Inf)
    eta = X[:, 1:] @ T[:, 1:].T + np.outer(X[:, 0], T[:, 0])
    sd, sigma, rho, ng = np.exp(eta[:, 0]), np.exp(eta[:, 0] / 2), np.exp(2 * eta[:, 1]), np.exp(eta[:, 5])
    ss = 1 / (1 + np.exp(-eta[:, 4]))
    nus = (hi - lo) * ss + lo
    dl = (hi - lo) * ss * (1 - ss) / (2 * nus)      # d log nu_ij / d eta_smooth of one side
    off = rows != cols
    i, j = rows[off], cols[off]
    if mode == "geom":
        nu = np.sqrt(nus[i]) * np.sqrt(nus[j])
    elif mode == "geom0":
        nu = np.zeros(i.size)
    else:
        nu = np.full(i.size, float(nu_fixed))
    h = np.sqrt(((locs[i] - locs[j]) ** 2).sum(axis=1))
    u = np.sqrt(8 * nu) * h / np.sqrt((rho[i] + rho[j]) / 2)
    coinc = u <= EPS
    far = u >= 706
    live = ~coinc & ~far
    M, Mu, Mn = np.zeros(i.size), np.zeros(i.size), np.zeros(i.size)
    M[live], Mu[live], Mn[live] = matern_and_partials(nu[live], u[live], "geom" if mode.startswith("geom") else mode)
    if not smooth_free:
        Mn[:] = 0
    P = 2 * np.sqrt(rho[i] * rho[j]) / (rho[i] + rho[j]) * sigma[i] * sigma[j]
    C = P * M
    own = (sd + ng)[np.maximum(i, j)]
    vals = np.empty(rows.size)
    vals[~off] = (sd + ng)[rows[~off]]
    vals[off] = np.where(coinc, own, C)
    S = np.zeros((n, n))
    S[rows, cols] = np.asarray(te, dtype=np.float64) * vals
    info = dict(rows=rows, cols=cols, off=off, i=i, j=j, coinc=coinc, live=live, C=np.where(live, C, 0.0),
                U=np.where(live, P * Mu * u, 0.0), Sm=np.where(live, P * Mn * nu, 0.0), rho=rho, sd=sd, ng=ng, dl=dl,
                smooth_free=smooth_free, te=np.asarray(te, dtype=np.float64))
    return S, info


def neg2loglik_taper_grad(T, mean, locs, X, z, smooth_limits, ref_taper):
    """(f, parts, grad_logdet 6 x p, grad_quad 6 x p, grad_mean p): parts = (log det S / 2, the r quadratic forms); the
    gradient of f is grad_logdet + grad_quad."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    Z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    r = Z.shape[1]
    S, q = taper_matrix(T, locs, X, smooth_limits, ref_taper)
    R = Z - (X @ np.asarray(mean, dtype=np.float64))[:, None]
    cf = linalg.cho_factor(S, lower=True)
    Sinv = linalg.cho_solve(cf, np.eye(n))
    A = Sinv @ R
    half_logdet = float(np.sum(np.log(np.diag(cf[0]))))
    quads = np.sum(R * A, axis=0)
    f = r * (n * np.log(2 * np.pi) + 2 * half_logdet) + float(np.sum(quads))
    rows, cols, off, i, j = q["rows"], q["cols"], q["off"], q["i"], q["j"]
    out = []
    for W in (r * Sinv, -(A @ A.T)):
        wt_off = W[i, j] * q["te"][off]              # every ordered pair of the symmetric pattern
        wt_diag = W[rows[~off], cols[~off]] * q["te"][~off]
        g = np.zeros((6, n))
        # the row site's partial of an ordinary entry; the ordered pair (j, i) brings the column site's
        phi = q["rho"][i] / (q["rho"][i] + q["rho"][j])
        g[0] += np.bincount(i, 2 * wt_off * 0.5 * q["C"], minlength=n)
        g[1] += np.bincount(i, 2 * wt_off * (q["C"] * (1 - 2 * phi) - q["U"] * phi), minlength=n)
        if q["smooth_free"]:
            g[4] += np.bincount(i, 2 * wt_off * (q["Sm"] + q["U"] / 2) * q["dl"][i], minlength=n)
        # a coincident pair is the diagonal value of its larger-index site
        cl = q["coinc"] & (i > j)
        g[0] += np.bincount(i, np.where(cl, 2 * wt_off * q["sd"][i], 0.0), minlength=n)
        g[5] += np.bincount(i, np.where(cl, 2 * wt_off * q["ng"][i], 0.0), minlength=n)
        d = rows[~off]
        g[0] += np.bincount(d, wt_diag * q["sd"][d], minlength=n)
        g[5] += np.bincount(d, wt_diag * q["ng"][d], minlength=n)
        out.append((X.T @ g.T).T.copy())
    gm = -2 * X.T @ A.sum(axis=1)
    return f, np.concatenate([[half_logdet], quads]), out[0], out[1], gm


# --------------------------------------------------------------------------- #
def tile_envelope(rows, cols, n, tile):
    """hi[c] (one past the last tile row of tile column c) of a symmetric pattern: at least the diagonal tile, monotone."""
    nt = (n + tile - 1) // tile
    hi = np.arange(1, nt + 1)
    first = np.full(n, n)
    np.minimum.at(first, rows, cols)
    for i in range(n):
        c0, ti = min(first[i], i) // tile, i // tile
        hi[c0:ti + 1] = np.maximum(hi[c0:ti + 1], ti + 1)
    return np.maximum.accumulate(hi)


def selinv_envelope(S, tile, hi, symmetric=True):
    """Z = S^-1 on the envelope tiles (elsewhere NaN) by the sweep J = nt-1 .. 0 over the band factor:
    G_KJ = L_KJ L_JJ^-1,  Z_IJ = -sum_K Z_IK G_KJ,  Z_JJ = L_JJ^-T L_JJ^-1 - sum_K Z_KJ' G_KJ  (J < I, K < hi[J]).
    The diagonal tile is symmetrised, as the library does: the equations determine Z only together with its symmetry, and
    the rounding-level antisymmetric part of a diagonal tile is a solution of the sweep that grows (symmetric=False shows it)."""
    n = S.shape[0]
    nt = (n + tile - 1) // tile
    L = np.linalg.cholesky(S)
    sl = [slice(t * tile, min(n, (t + 1) * tile)) for t in range(nt)]
    Z = np.full((n, n), np.nan)
    for J in range(nt - 1, -1, -1):
        Ks = list(range(J + 1, hi[J]))
        assert not np.any(L[sl[hi[J] - 1].stop:, sl[J]]), "the factor leaves the envelope"
        W = np.linalg.inv(L[sl[J], sl[J]])
        G = {K: L[sl[K], sl[J]] @ W for K in Ks}
        for I in Ks:
            acc = np.zeros((sl[I].stop - sl[I].start, sl[J].stop - sl[J].start))
            for K in Ks:
                Zik = Z[sl[I], sl[K]] if I >= K else Z[sl[K], sl[I]].T
                acc -= Zik @ G[K]
            Z[sl[I], sl[J]] = acc
        D = W.T @ W
        for K in Ks:
            D -= Z[sl[K], sl[J]].T @ G[K]
        Z[sl[J], sl[J]] = (D + D.T) / 2 if symmetric else D
    return Z
