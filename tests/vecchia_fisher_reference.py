"""Numpy statement of the expected information of the Vecchia likelihood (cocons_fisher_vecchia) on
fisher_reference's matrices (test infrastructure, not a test module).

For observation i with neighbours j_1 < .. < j_k: C = Sigma[(j.., i), (j.., i)] and C_a the same block of Sigma_a
(fisher_reference.sigma_and_directions: the dense conventions, a coincident pair on the EARLIER row's diagonal partials -- its
ii < jj is the block kernel's orientation, because a block's rows ascend in the caller's index).  Two statements:

  block difference   sum_i [ info_solve(C, C_a) - info_solve(C_NN, C_a,NN) ]       (NN: the block without its last row)
  last row           sum_i [ sum_{j < k} g_a[j] g_b[j] + g_a[k] g_b[k] / 2 ],  g_a = L^-1 (C_a s),  s = L^-T e_k,  C = L L'

and info_mean = r sum_i u_i u_i', u_i = s' X[(j.., i)].  Both times r."""
import numpy as np

import fisher_reference as FR
from vecchia_reference import rows_of


def setup(n, seed=3, p=3):
    """(locs, X, theta): uniform sites in no spatial order, the design and theta of test_gpu_fisher._setup"""
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(wl.design_from_locs(locs)["std.covs"][:, :p])
    th = wl.theta_full(scale0=np.log(0.2))
    for k in th:
        th[k] = np.array(th[k][:p], dtype=float)
    th["mean"] = np.array([0.3, -0.15, 0.2])[:p]
    return locs, X, th


def info_blocks(Sigma, Sa, nn, r=1):
    """the block-difference statement"""
    n, nd = Sigma.shape[0], Sa.shape[0]
    info = np.zeros((nd, nd))
    for i in range(n):
        nb = rows_of(nn, i)
        idx = np.append(nb, i)
        info += FR.info_solve(Sigma[np.ix_(idx, idx)], Sa[:, idx[:, None], idx[None, :]], r)
        if nb.size:
            info -= FR.info_solve(Sigma[np.ix_(nb, nb)], Sa[:, nb[:, None], nb[None, :]], r)
    return info


def info_last_row(Sigma, Sa, nn, r=1, X=None, rows=None, batch=256):
    """the last-row statement, rows of equal block size together: (info, info_mean or None); rows: the observations summed
    over (default all)"""
    n, nd = Sigma.shape[0], Sa.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    blocks = {}
    for i in rows:
        blocks.setdefault(rows_of(nn, i).size, []).append(np.append(rows_of(nn, i), i))
    info = np.zeros((nd, nd))
    info_mean = None if X is None else np.zeros((X.shape[1], X.shape[1]))
    for k, lst in sorted(blocks.items()):
        w = np.ones(k + 1)
        w[k] = 0.5
        e = np.zeros((k + 1, 1))
        e[k] = 1.0
        for b0 in range(0, len(lst), batch):
            idx = np.array(lst[b0:b0 + batch])                               # nb x (k + 1)
            L = np.linalg.cholesky(Sigma[idx[:, :, None], idx[:, None, :]])
            s = np.linalg.solve(np.swapaxes(L, 1, 2), e[None])               # nb x (k + 1) x 1
            q = np.stack([Sa[a][idx[:, :, None], idx[:, None, :]] @ s for a in range(nd)], axis=-1)[:, :, 0, :]
            g = np.linalg.solve(L, q)                                        # nb x (k + 1) x nd
            info += np.einsum("nja,njb,j->ab", g, g, w)
            if X is not None:
                u = np.einsum("nj,njp->np", s[:, :, 0], X[idx])
                info_mean += u.T @ u
    return r * info, (None if X is None else r * info_mean)


def statement(T, locs, X, smooth_limits, dirs, nn, r=1, rows=None):
    """(info, info_mean) by the last-row statement from the table T"""
    S, Sa = FR.sigma_and_directions(T, locs, X, smooth_limits, dirs)
    return info_last_row(S, Sa, nn, r, np.asarray(X, dtype=float), rows)


def banded_table(n, m):
    """row i names its m predecessors i - 1 .. i - m (1-based, 0 = none)"""
    nn = np.zeros((n, m), dtype=np.int32, order="F")
    for j in range(m):
        nn[j + 1:, j] = np.arange(1, n - j)
    return nn


def statement_banded(T, locs, X, smooth_limits, dirs, m, r=1, seg=400):
    """`statement` for banded_table(n, m) at an n too large for an n x n matrix: segment by segment, every block inside the
    dense matrices of seg + m consecutive sites"""
    n = X.shape[0]
    info = info_mean = 0.0
    for a in range(0, n, seg):
        lo, hi = max(a - m, 0), min(a + seg, n)
        I, Im = statement(T, locs[lo:hi], X[lo:hi], smooth_limits, dirs, banded_table(hi - lo, m), r, np.arange(a - lo, hi - lo))
        info, info_mean = info + I, info_mean + Im
    return info, info_mean
