"""Independent numpy / scipy statement of the expected (Fisher) information of a tapered fit (test infrastructure).

S = T o C(theta) on a symmetric CSR pattern as grad_taper_reference.taper_matrix assembles it, and for a direction v (a 6 x p
table) S_v = T o sum_tk v[t, k] dC / dtheta[t, k] on the same pattern, from the per-entry numbers of taper_matrix under the
taper gradient's conventions: the FULL scale vector (rho_i = e^(2 eta_scale,i), factor 1, no global range), a coincident
pair takes the diagonal value of the site with the larger index, u >= 706 contributes 0, the aniso and tilt rows do not enter.
With the site weights w[f] = X v[f] an ordinary entry (i, j) is

    T_ij [ C/2 (w_sd,i + w_sd,j) + (C (1 - 2 phi_i) - U phi_i) w_sc,i + (C (1 - 2 phi_j) - U phi_j) w_sc,j
           + (Sm + U/2) (dl_i w_sm,i + dl_j w_sm,j) ],     phi_i = rho_i / (rho_i + rho_j),

and a diagonal or coincident one T_ij (sd_m w_sd,m + g_m w_ng,m).  Then I[a, b] = (r / 2) tr(S^-1 S_a S^-1 S_b) by
fisher_reference.info_whiten / info_solve, and -- band_fisher -- by the sweep the library runs on the band factor: probe
rows through a backward right-looking solve, the sparse product per direction, a forward right-looking solve and per-strip
Gram sums, on tiles with an envelope.
"""
from __future__ import annotations

import os
import sys

import numpy as np
from scipy import linalg, sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_taper_reference as GT  # noqa: E402
from fisher_reference import info_solve, info_whiten, metric, scaling_direction  # noqa: E402,F401
from krige_taper_reference import envelope  # noqa: E402


def _lower_mirrored(A):
    return np.tril(A) + np.tril(A, -1).T


def direction_matrices(T, locs, X, smooth_limits, ref_taper, dirs):
    """(S n x n, S_a ndir x n x n) dense, zero off the pattern; the lower triangle mirrored, as the library reads the
    pattern (the two orders of a product of four site factors differ in the last bit)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    S, q = GT.taper_matrix(T, locs, X, smooth_limits, ref_taper)
    rows, cols, off, i, j = q["rows"], q["cols"], q["off"], q["i"], q["j"]
    te, rho, sd, ng, dl = q["te"], q["rho"], q["sd"], q["ng"], q["dl"]
    C, U, Sm, coinc = q["C"], q["U"], q["Sm"], q["coinc"]
    phi_i = rho[i] / (rho[i] + rho[j])
    phi_j = rho[j] / (rho[i] + rho[j])
    own = np.maximum(i, j)
    V = np.asarray(dirs, dtype=np.float64).reshape(-1, 6, p)
    Sa = np.zeros((V.shape[0], n, n))
    for a, v in enumerate(V):
        w = X @ v.T                                  # n x 6: sd, scale, aniso, tilt, smooth, nugget
        site = sd * w[:, 0] + ng * w[:, 5]           # derivative of the diagonal value sd_m + g_m
        e = (0.5 * C * (w[i, 0] + w[j, 0]) + (C * (1 - 2 * phi_i) - U * phi_i) * w[i, 1]
             + (C * (1 - 2 * phi_j) - U * phi_j) * w[j, 1])
        if q["smooth_free"]:
            e = e + (Sm + U / 2) * (dl[i] * w[i, 4] + dl[j] * w[j, 4])
        vals = np.empty(rows.size)
        vals[~off] = site[rows[~off]]
        vals[off] = np.where(coinc, site[own], e)
        Sa[a][rows, cols] = te * vals
        Sa[a] = _lower_mirrored(Sa[a])
    return _lower_mirrored(S), Sa


def info_mean(S, X, r=1):
    """r X' S^-1 X."""
    cf = linalg.cho_factor(S, lower=True)
    return r * (X.T @ linalg.cho_solve(cf, X))


def standard_directions(p):
    """The 3 p unit table entries of the std.dev, scale and smooth rows, the nugget intercept, and v_s = e_sd,0 + e_ng,0
    (S_{v_s} = S): 3 p + 2 directions, the last one dependent on the others."""
    out = []
    for t in (0, 1, 4):
        for k in range(p):
            v = np.zeros((6, p))
            v[t, k] = 1.0
            out.append(v)
    v = np.zeros((6, p))
    v[5, 0] = 1.0
    out.append(v)
    out.append(scaling_direction(p))
    return np.stack(out)


def band_fisher(S, Sa, probes, pivot, r=1, weight=None, X=None, tile=128, strip=64):
    """The library's sweep in numpy.  pivot: 1-based observation per position of the order the factor is taken in
    (cocons_fit_taper_order); probes: n x N, column k probe k in the observations' order.  Returns (info, info_mean or None,
    hi, W): info = weight * sum over the strips of the per-strip Gram sums (weight None: r / (2 N))."""
    n = S.shape[0]
    piv = np.asarray(pivot, dtype=np.int64) - 1
    npad = (n + tile - 1) // tile * tile
    nt = npad // tile
    Sp = np.eye(npad)
    Sp[:n, :n] = S[np.ix_(piv, piv)]
    L = np.linalg.cholesky(Sp)
    L[np.abs(L) < 1e-300] = 0.0
    hi, W = envelope(L, tile)
    lo = [min(K for K in range(nt) if hi[K] > J) for J in range(nt)]
    sl = [slice(t * tile, (t + 1) * tile) for t in range(nt)]
    P = np.asarray(probes, dtype=np.float64).reshape(n, -1)
    N = P.shape[1]
    rows = (N + strip - 1) // strip * strip
    E = np.zeros((rows, npad))
    E[:N, :n] = P[piv].T
    # backward right-looking solve: W = E L^-1
    for J in range(nt - 1, -1, -1):
        E[:, sl[J]] = linalg.solve_triangular(L[sl[J], sl[J]], E[:, sl[J]].T, lower=True, trans="T").T
        for K in range(lo[J], J):
            E[:, sl[K]] -= E[:, sl[J]] @ L[sl[J], sl[K]]
    # the CSR product per direction, then the forward right-looking solve Q = U L^-T of every direction's rows
    Q = []
    mats = [sparse.csr_matrix(A[np.ix_(piv, piv)]) for A in Sa]
    extra = [] if X is None else [np.asarray(X, dtype=np.float64)[piv].T]
    for k, src in enumerate(mats + extra):
        Uq = np.zeros((E.shape[0] if k < len(mats) else src.shape[0], npad))
        Uq[:, :n] = (src @ E[:, :n].T).T if k < len(mats) else src      # (S_a symmetric: W S_a = (S_a W')')
        for J in range(nt):
            Uq[:, sl[J]] = linalg.solve_triangular(L[sl[J], sl[J]], Uq[:, sl[J]].T, lower=True).T
            for I in range(J + 1, hi[J]):
                Uq[:, sl[I]] -= Uq[:, sl[J]] @ L[sl[I], sl[J]].T
        Q.append(Uq)
    nd = len(mats)
    info = np.zeros((nd, nd))
    for s0 in range(0, rows, strip):
        part = np.zeros((nd, nd))
        for a in range(nd):
            for b in range(a, nd):
                part[a, b] = part[b, a] = np.sum(Q[a][s0:s0 + strip] * Q[b][s0:s0 + strip])
        info += part
    info *= (0.5 * r / N) if weight is None else weight
    im = None if X is None else r * (Q[-1] @ Q[-1].T)
    return info, im, hi, W
