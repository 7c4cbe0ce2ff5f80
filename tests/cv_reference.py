"""The numpy statement of cross-validated kriging, twice (what cocons_cv_dense / cocons_cv_taper are checked against).

For a covariance S of the n observations, residuals R = z - X mean (n x r) and fold labels lab (n integers), every
observation is predicted from the observations outside its fold:

  cv_brute   per fold B with complement A:  e_B = R_B - S_BA S_AA^-1 R_A,  var_B = diag(S_BB - S_BA S_AA^-1 S_AB)
             -- one Cholesky of S_AA per fold, nothing shared between folds;
  cv_kroute  with K = S^-1 and U = K R:     e_B = (K_BB)^-1 U_B,           var_B = diag((K_BB)^-1)
             -- one inverse, then one small block per fold (the route the library takes).

Both return (e n x r, var n).  gaps() measures a result against a reference in the units of the task:
gap_e = max |e - e_ref| / sd_ref (sd_ref = sqrt(var_ref), per observation), gap_v = max |var - var_ref| / var_ref."""
from __future__ import annotations

import numpy as np
from scipy import linalg


def cv_brute(S, R, lab):
    S = np.asarray(S, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(S.shape[0], -1)
    lab = np.asarray(lab)
    e, var = np.empty_like(R), np.empty(S.shape[0])
    for l in np.unique(lab):
        B = np.nonzero(lab == l)[0]
        A = np.nonzero(lab != l)[0]
        cf = linalg.cho_factor(S[np.ix_(A, A)], lower=True)
        sol = linalg.cho_solve(cf, np.column_stack([R[A], S[np.ix_(A, B)]]))
        r = R.shape[1]
        e[B] = R[B] - S[np.ix_(B, A)] @ sol[:, :r]
        var[B] = np.diag(S[np.ix_(B, B)]) - np.einsum("ij,ji->i", S[np.ix_(B, A)], sol[:, r:])
    return e, var


def cv_kroute(S, R, lab):
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    R = np.asarray(R, dtype=np.float64).reshape(n, -1)
    lab = np.asarray(lab)
    K = linalg.cho_solve(linalg.cho_factor(S, lower=True), np.eye(n))
    K = (K + K.T) / 2
    U = K @ R
    e, var = np.empty_like(R), np.empty(n)
    for l in np.unique(lab):
        B = np.nonzero(lab == l)[0]
        cf = linalg.cho_factor(K[np.ix_(B, B)], lower=True)
        e[B] = linalg.cho_solve(cf, U[B])
        var[B] = np.diag(linalg.cho_solve(cf, np.eye(B.size)))
    return e, var


def gaps(e, var, e_ref, var_ref):
    e, e_ref = np.asarray(e).reshape(len(var_ref), -1), np.asarray(e_ref).reshape(len(var_ref), -1)
    gap_e = float(np.max(np.abs(e - e_ref) / np.sqrt(var_ref)[:, None]))
    gap_v = float(np.max(np.abs(np.asarray(var) - var_ref) / var_ref))
    return gap_e, gap_v


def _apart(lab, i, j):
    """labels with observations i and j in different folds: j trades places with the first observation of another fold
    (the fold sizes stay)"""
    lab = np.array(lab)
    if lab[i] == lab[j]:
        k = next(k for k in range(lab.size) if lab[k] != lab[i] and k != i)
        lab[j], lab[k] = lab[k], lab[j]
    return lab


def layouts(locs, seed=11, pair=(3, 7)):
    """The four fold layouts of the task for n locations in the unit square: leave-one-out, 10 random folds of equal size,
    16 spatial blocks (4 x 4), 2 random folds of equal size -- each with the observations `pair` in different folds (the
    coincident pair of the test problem: the smallest predictive variance is there)."""
    locs = np.asarray(locs)
    n = locs.shape[0]
    rng = np.random.default_rng(seed)
    out = {"loo": np.arange(n)}
    out["random10"] = _apart(rng.permutation(n) % 10, *pair)
    cell = np.minimum((locs * 4).astype(int), 3)
    blocks = cell[:, 0] * 4 + cell[:, 1]
    if blocks[pair[0]] == blocks[pair[1]]:
        blocks[pair[1]] = (blocks[pair[1]] + 1) % 16
    out["spatial16"] = blocks
    out["two"] = _apart(rng.permutation(n) % 2, *pair)
    return out


_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def crps_integral(z, mu, sd, width=40.0, steps=400001):
    """the definition of the CRPS of N(mu, sd^2) at z, integral of (F(x) - 1{x >= z})^2 dx, by the trapezoid rule with the
    kink at z on the grid"""
    from scipy.stats import norm
    total = 0.0
    for lo, hi, ind in ((z - width * sd, z, 0.0), (z, z + width * sd, 1.0)):
        x = np.linspace(lo, hi, steps)
        total += _trapezoid((norm.cdf(x, mu, sd) - ind) ** 2, x)
    return float(total)
