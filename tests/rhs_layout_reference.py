"""Plain statement of what the value entries return when many right-hand sides ride through one factorisation (test
infrastructure): the dense, Profile and REML -2 log-likelihood cores and their `parts`, in the C ABI's order, from the
oracle's long-double Cholesky (oracle.chol_ld) and a Gram matrix summed in long double.

    S = cov_rns(theta),   Y = L^-1 [Z - X mean | Xb]  (Profile / REML: no mean),   G = Y' Y
    dense:           sum_k  n log 2 pi + 2 ld + G_kk                                      parts = [ld, G_kk ...]
    Profile / REML:  W = G[r:, r:], g_k = G[r:, k], quad_k = G_kk - g_k' W^-1 g_k, ldW = sum log diag chol(W),
                     betas = W^-1 mean_k(g_k),
                     sum_k  n_eff log 2 pi + 2 ld (+ 2 ldW) + quad_k                      parts = [ld, ldW, quad ..., betas ...]
                     n_eff = n (Profile) or n - rank(X) (REML, Xb = X)

The reference asserts the conditions under which agreeing with it means something: the factorisation succeeds, W is well
conditioned (cond < 1e4) and the subtraction in quad_k cancels at most one bit (g_k' W^-1 g_k <= G_kk / 2).  The small solves
with W (at most 32 x 32) run in long double too.  tests/test_rhs_layout_reference.py pins all three forms to the oracle's
literal restatements of the R closures."""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble


def layout_problem(n, p, r, seed):
    """The problems of tests/test_gpu_rhs_layouts.py: _general_problem of tests/test_gpu_grad.py (uniform locations, an
    intercept and p - 1 covariates x 0.3, a nugget covariate effect) with r realisations that carry a trend,
    z = N(0, 1) + X b, b = 0.3 N(0, 1); x_betas = X."""
    from test_gpu_grad import _general_problem
    locs, X, th, _ = _general_problem(n, p, 1, seed)
    rng = np.random.default_rng(seed + 1)
    b = 0.3 * rng.standard_normal(p)
    z = rng.standard_normal((n, r)) + (X @ b)[:, None]
    return locs, X, th, z


def _chol_ld_small(W):
    """Lower Cholesky factor of a small matrix in long double."""
    q = W.shape[0]
    C = np.zeros((q, q), dtype=LD)
    for j in range(q):
        d = W[j, j] - np.dot(C[j, :j], C[j, :j])
        assert d > 0, "W is not positive definite"
        C[j, j] = np.sqrt(d)
        C[j + 1:, j] = (W[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    return C


def _solve_ld_small(C, B):
    """W^-1 B from W = C C' in long double (B: q x k)."""
    q = C.shape[0]
    Y = np.array(B, dtype=LD, copy=True)
    for i in range(q):
        Y[i] = (Y[i] - C[i, :i] @ Y[:i]) / C[i, i]
    for i in range(q - 1, -1, -1):
        Y[i] = (Y[i] - C[i + 1:, i] @ Y[i + 1:]) / C[i, i]
    return Y


def gram(oracle, th, locs, X, rhs, smooth_limits):
    """(ld, G): sum log diag chol(S) and the long-double Gram matrix of L^-1 rhs.  Asserts info == 0."""
    S = oracle.cov_rns(th, locs, X, smooth_limits)
    info, ld, _, Y = oracle.chol_ld(S, rhs)
    assert info == 0, info
    Y = np.asarray(Y, dtype=LD)
    return ld, Y.T @ Y


def dense(oracle, th, locs, X, z, smooth_limits):
    """(value, parts[1 + r]) of cocons_neg2loglik_dense."""
    n = X.shape[0]
    Z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    ld, G = gram(oracle, th, locs, X, Z - (X @ np.asarray(th["mean"], dtype=np.float64))[:, None], smooth_limits)
    quad = np.diag(G)
    total = sum(LD(n) * LD(math.log(2 * math.pi)) + 2 * LD(ld) + q for q in quad)
    return float(total), np.r_[ld, quad.astype(np.float64)]


def profile(oracle, th, locs, X, z, x_betas, smooth_limits, reml=False, check=True, ld_gram=None):
    """(value, parts[2 + r + nxb], conditions) of cocons_neg2loglik_profile (Xb = x_betas) or, reml=True, of
    cocons_neg2loglik_reml (Xb = X, n_eff = n - matrix_rank(X)).  conditions = {"cond_W", "ratio"}; with check they are
    asserted (cond(W) < 1e4, max_k g_k' W^-1 g_k / G_kk <= 0.5).  ld_gram: what gram() returned for [Z | Xb], when the caller
    has it already (Profile and REML with x_betas = X read the same one)."""
    n = X.shape[0]
    Z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    Xb = np.asarray(X if reml else x_betas, dtype=np.float64).reshape(n, -1)
    r = Z.shape[1]
    ld, G = ld_gram if ld_gram is not None else gram(oracle, th, locs, X, np.column_stack([Z, Xb]), smooth_limits)
    W, g = G[r:, r:], G[r:, :r]
    C = _chol_ld_small(W)
    Wg = _solve_ld_small(C, g)
    corr = np.sum(g * Wg, axis=0)
    Gkk = np.diag(G)[:r]
    quad = Gkk - corr
    ldW = np.sum(np.log(np.diag(C)))
    betas = _solve_ld_small(C, g.mean(axis=1)[:, None])[:, 0]
    n_eff = n - int(np.linalg.matrix_rank(X)) if reml else n
    total = sum(LD(n_eff) * LD(math.log(2 * math.pi)) + 2 * LD(ld) + (2 * ldW if reml else 0) + q for q in quad)
    cond = {"cond_W": float(np.linalg.cond(W.astype(np.float64))), "ratio": float(np.max(corr / Gkk))}
    if check:
        assert cond["cond_W"] < 1e4, cond
        assert cond["ratio"] <= 0.5, cond
    parts = np.r_[ld, float(ldW), quad.astype(np.float64), betas.astype(np.float64)]
    return float(total), parts, cond
