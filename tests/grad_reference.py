"""Independent numpy / scipy statement of the analytic gradient of the dense -2 log-likelihood (test infrastructure).

f = sum_c [ n log 2 pi + log det Sigma + r_c' Sigma^-1 r_c ],  r_c = z_c - X mean, Sigma = cov_rns(theta) in the caller's
order.  W = r Sigma^-1 - A A' (A = Sigma^-1 R); df/dtheta_a = sum_ij W_ij dSigma_ij/dtheta_a, df/dmean = -2 X' A 1.
Pair partials from the closed form of every entry, scipy.special.kv / kvp for the Matern part and a Richardson central
difference in nu for its order derivative.
"""
from __future__ import annotations

import math

import numpy as np
from scipy import linalg, special

EPS = 2.220446049250313e-16


def select_mode(T, smooth_limits):
    """(mode, nu_fixed, smooth_free): 'half' / 'threehalf' / 'fivehalf' / 'geom' as the library selects them."""
    lo, hi = smooth_limits
    if np.all(T[4, 1:] == 0) and lo == hi:
        for name, v in (("half", 0.5), ("threehalf", 1.5), ("fivehalf", 2.5)):
            if abs(lo - v) < 1e-6:
                return name, lo, False
        return "geom0", lo, False
    return "geom", None, hi != lo


def _matern(nu, u):
    return 2.0 ** (1 - nu) / special.gamma(nu) * u ** nu * special.kv(nu, u)


def matern_and_partials(nu, u, mode="geom"):
    """M, dM/du, dM/dnu (arrays)."""
    nu = np.broadcast_to(np.asarray(nu, dtype=np.float64), np.shape(u))
    u = np.asarray(u, dtype=np.float64)
    e = np.exp(-u)
    if mode == "half":
        return e, -e, np.zeros_like(u)
    if mode == "threehalf":
        return (1 + u) * e, -u * e, np.zeros_like(u)
    if mode == "fivehalf":
        return (1 + u + u * u / 3) * e, -(u / 3) * (1 + u) * e, np.zeros_like(u)
    c = 2.0 ** (1 - nu) / special.gamma(nu)
    M = c * u ** nu * special.kv(nu, u)
    Mu = c * (nu * u ** (nu - 1) * special.kv(nu, u) + u ** nu * special.kvp(nu, u))
    h = 1e-3 * nu
    d1 = (_matern(nu + h, u) - _matern(nu - h, u)) / (2 * h)
    d2 = (_matern(nu + h / 2, u) - _matern(nu - h / 2, u)) / h
    Mn = (4 * d2 - d1) / 3
    return M, Mu, Mn


def site_quantities(T, X, smooth_limits):
    lo, hi = smooth_limits
    eta = X @ T.T                                  # n x 6: sd, scale, aniso, tilt, smooth, nugget
    eta_rd = 2 * (X[:, 1:] @ T[1, 1:])
    q = dict(
        sd=np.exp(eta[:, 0]), sigma=np.exp(eta[:, 0] / 2), rd=np.exp(eta_rd), a=np.exp(eta[:, 2]),
        ng=np.exp(eta[:, 5]),
    )
    s = 1 / (1 + np.exp(-eta[:, 3]))
    q["t"] = math.pi * s
    q["tp"] = math.pi * s * (1 - s)
    ss = 1 / (1 + np.exp(-eta[:, 4]))
    q["nu"] = (hi - lo) * ss + lo
    q["dnu"] = (hi - lo) * ss * (1 - ss)
    return q


def neg2loglik_grad(T, mean, locs, X, z, smooth_limits):
    """(f, grad_table 6 x p, grad_mean p) in float64; T the 6 x p table."""
    T = np.asarray(T, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    n, p = X.shape
    Z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    nr = Z.shape[1]
    mode, nu_fixed, smooth_free = select_mode(T, smooth_limits)
    gr = math.exp(2 * T[1, 0])
    st = site_quantities(T, X, smooth_limits)
    ii, jj = np.tril_indices(n, -1)
    ii, jj = jj, ii                                # ii < jj: the first ("ii") location is the lower index
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
    far = u >= 706
    live = ~coinc & ~far
    ul, nul = u[live], nu[live]
    M = np.zeros_like(u)
    Mu = np.zeros_like(u)
    Mn = np.zeros_like(u)
    M[live], Mu[live], Mn[live] = matern_and_partials(nul, ul, "geom" if mode.startswith("geom") else mode)
    if not smooth_free:
        Mn[:] = 0
    P = st["sigma"][ii] * st["sigma"][jj] * np.sqrt(ra[ii] * sn[ii] * ra[jj] * sn[jj] / D)
    C = M * P
    Sigma = np.diag(st["sd"] + st["ng"])
    off = np.where(coinc, (st["sd"] + st["ng"])[ii], C)
    Sigma[ii, jj] = off
    Sigma[jj, ii] = off
    # objective
    R = Z - (X @ np.asarray(mean, dtype=np.float64))[:, None]
    cf = linalg.cho_factor(Sigma, lower=True)
    Sinv = linalg.cho_solve(cf, np.eye(n))
    A = Sinv @ R
    logdet = 2 * np.sum(np.log(np.diag(cf[0])))
    f = nr * (n * math.log(2 * math.pi) + logdet) + float(np.sum(R * A))
    W = nr * Sinv - A @ A.T
    w2 = 2 * W[ii, jj]
    # partials with respect to the site predictors of each side
    with np.errstate(divide="ignore", invalid="ignore"):
        U = np.where(live, P * Mu * u, 0.0)
        Cl = np.where(live, C, 0.0)
    g = np.zeros((6, n))
    for side in (ii, jj):
        rdi, ai, rai, cti, sni, tpi = rd[side], a[side], ra[side], ct[side], sn[side], st["tp"][side]
        parts = (
            (1, rdi / 2, rdi * ai ** 2 / 2, rai * cti / 2, 0.5),
            (2, 0.0, rdi * ai ** 2, rai * cti / 2, 0.5),
            (3, 0.0, 0.0, -rai * sni * tpi / 2, 0.5 * cti / sni * tpi),
        )
        for fam, s11p, s22p, s12p, amp in parts:
            Dp = s11p * s22 + s11 * s22p - 2 * s12 * s12p
            qp = s22p * dx * dx + s11p * dy * dy - 2 * s12p * dx * dy
            with np.errstate(divide="ignore", invalid="ignore"):
                d = U * 0.5 * (qp / q - Dp / D) + Cl * (amp - 0.5 * Dp / D)
            d = np.where(live, d, 0.0)
            g[fam] += np.bincount(side, w2 * d, minlength=n)
        g[0] += np.bincount(side, w2 * 0.5 * Cl, minlength=n)
        if smooth_free:
            dl = st["dnu"][side] / (2 * st["nu"][side])
            d = np.where(live, P * Mn * nu * dl + U * 0.5 * dl, 0.0)
            g[4] += np.bincount(side, w2 * d, minlength=n)
    # coincident pairs: the ii site's diagonal value
    g[0] += np.bincount(ii, np.where(coinc, w2 * st["sd"][ii], 0.0), minlength=n)
    g[5] += np.bincount(ii, np.where(coinc, w2 * st["ng"][ii], 0.0), minlength=n)
    dW = np.diag(W)
    g[0] += dW * st["sd"]
    g[5] += dW * st["ng"]
    gt = X.T @ g.T                                 # p x 6
    gt = gt.T.copy()
    gt[1, 1:] *= 2
    gt[1, 0] = float(np.sum(w2 * -U))
    gm = -2 * X.T @ A.sum(axis=1)
    return f, gt, gm

