"""Independent numpy / scipy statement of the expected information of the REML fit (test infrastructure), on top of
tests/fisher_reference.py (Sigma and the direction matrices Sigma_a; imported, left untouched).

With X the design the REML objective profiles out, V = Sigma^-1 X, W = X' V and P = Sigma^-1 - V W^-1 V'
(R/neg2loglikelihood.R:273-278), I_R[a, b] = (r / 2) tr(P Sigma_a P Sigma_b).  Two forms:
  info_projector  (r / 2) sum (P Sigma_a) o (P Sigma_b)' with P formed as written;
  info_contrasts  the ML information of the error contrasts K' z, K an orthonormal basis of null(X'): the definition, and
                  independent of P.
"""
from __future__ import annotations

import numpy as np
from scipy import linalg

import fisher_reference as FR


def projector(Sigma, X):
    """P = Sigma^-1 - V W^-1 V' by Cholesky solves, symmetrised."""
    X = np.asarray(X, dtype=np.float64)
    cf = linalg.cho_factor(Sigma, lower=True)
    Si = linalg.cho_solve(cf, np.eye(Sigma.shape[0]))
    V = linalg.cho_solve(cf, X)
    W = X.T @ V
    P = Si - V @ linalg.cho_solve(linalg.cho_factor(W, lower=True), V.T)
    return 0.5 * (P + P.T)


def info_projector(Sigma, Sa, X, r=1):
    """(r / 2) sum G_a o G_b' with G_a = P Sigma_a."""
    P = projector(Sigma, X)
    G = np.stack([P @ S for S in Sa])
    nd = G.shape[0]
    return 0.5 * r * (G.reshape(nd, -1) @ np.ascontiguousarray(G.transpose(0, 2, 1)).reshape(nd, -1).T)


def contrast_basis(X):
    """K (n x (n - rank X)), orthonormal, K' X = 0: the trailing columns of the full QR of X."""
    X = np.asarray(X, dtype=np.float64)
    Q, _ = np.linalg.qr(X, mode="complete")
    return Q[:, np.linalg.matrix_rank(X):]


def info_contrasts(Sigma, Sa, X, r=1):
    """The ML information of K' z ~ N(0, K' Sigma K): FR.info_solve on the contrasts' matrices."""
    K = contrast_basis(X)
    return FR.info_solve(K.T @ Sigma @ K, np.stack([K.T @ S @ K for S in Sa]), r)
