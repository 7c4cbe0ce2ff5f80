"""Independent numpy statement of the analytic gradients of the Profile and REML -2 log-likelihoods (test infrastructure).

The contraction df/dtheta_a = sum_ij W_ij dSigma_ij/dtheta_a is linear in W, and grad_reference.neg2loglik_grad(T, 0, ..., Y)
contracts W = k Sigma^-1 - (Sigma^-1 Y)(Sigma^-1 Y)' for an n x k matrix Y.  With beta = (Xb' Sigma^-1 Xb)^-1 Xb' Sigma^-1 Z and
L = chol(Xb' Sigma^-1 Xb):

    Profile:  W = r Sigma^-1 - U U',  U = Sigma^-1 (Z - Xb beta)            ->  g(Z - Xb beta)
    REML:     W = r Sigma^-1 - U U' - r C C',  C = Sigma^-1 Xb L^-T         ->  g(Z - X beta) + r [ g(X L^-T) - p g(0_{n x 1}) ]

(g(0) contracts Sigma^-1 alone).  Sigma comes from the CPU oracle; nothing of the library's host layer is used beyond theta_table.
Values: f = r (n_eff log 2 pi + log det Sigma [+ log det W]) + sum_k z_k' P z_k, n_eff = n (Profile) or n - rank(X) (REML).
"""
from __future__ import annotations

import math

import numpy as np

import grad_reference as GR


def _gls(theta_list, locs, X, Z, Xb, smooth_limits):
    from oracle import oracle as O
    O.build()
    S = O.cov_rns(theta_list, locs, X, smooth_limits)
    Lc = np.linalg.cholesky(S)
    V = np.linalg.solve(Lc.T, np.linalg.solve(Lc, Xb))
    W = Xb.T @ V
    beta = np.linalg.solve(W, V.T @ Z)
    Rz = Z - Xb @ beta
    quad = np.sum(Rz * np.linalg.solve(Lc.T, np.linalg.solve(Lc, Rz)), axis=0)
    logdet = 2 * float(np.sum(np.log(np.diag(Lc))))
    return W, beta, Rz, quad, logdet


def _table(theta_list):
    from cocons_amd.host import theta_table
    return theta_table(theta_list)


def profile_grad(theta_list, locs, X, z, x_betas, smooth_limits):
    """(f, grad_table 6 x p, beta q x r, quad r) of the Profile objective (no penalty)."""
    n, p = X.shape
    Z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    Xb = np.asarray(x_betas, dtype=np.float64).reshape(n, -1)
    r = Z.shape[1]
    W, beta, Rz, quad, logdet = _gls(theta_list, locs, X, Z, Xb, smooth_limits)
    _, gt, _ = GR.neg2loglik_grad(_table(theta_list), np.zeros(p), locs, X, Rz, smooth_limits)
    f = r * (n * math.log(2 * math.pi) + logdet) + float(np.sum(quad))
    return f, gt, beta, quad


def reml_grad(theta_list, locs, X, z, smooth_limits):
    """(f, grad_table 6 x p, beta p x r, quad r) of the REML objective (no penalty); Xb = X."""
    n, p = X.shape
    Z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    r = Z.shape[1]
    W, beta, Rz, quad, logdet = _gls(theta_list, locs, X, Z, X, smooth_limits)
    T, zero = _table(theta_list), np.zeros(p)
    Lw = np.linalg.cholesky(W)
    _, g_u, _ = GR.neg2loglik_grad(T, zero, locs, X, Rz, smooth_limits)
    _, g_c, _ = GR.neg2loglik_grad(T, zero, locs, X, np.linalg.solve(Lw, X.T).T, smooth_limits)
    _, g_0, _ = GR.neg2loglik_grad(T, zero, locs, X, np.zeros((n, 1)), smooth_limits)
    gt = g_u + r * (g_c - p * g_0)
    rank = int(np.linalg.matrix_rank(X))
    f = r * ((n - rank) * math.log(2 * math.pi) + logdet + 2 * float(np.sum(np.log(np.diag(Lw))))) + float(np.sum(quad))
    return f, gt, beta, quad
