"""Numpy statement of the grouped Vecchia information (cocons_fisher_vecchia_grouped) on fisher_reference's
matrices (test infrastructure, not a test module).

A block has the rows S ascending, the member set M, C = L L' and Z = L^-1.  The member at position p is
vecchia_fisher_reference's block on the leading p + 1 rows: s_p = L^-T e_p is row p of Z (supported on 0 .. p), and with
q_{a,p} = C_a[0..p, 0..p] s_p the vector g_{a,p} = L_{0..p}^-1 q_{a,p} is the leading p + 1 entries of column p of
G_a = Z C_a Z' -- L's leading sub-block is the factor of C's.  The block contributes

    info[a, b]      += sum_{p in M} ( sum_{j < p} G_a[j, p] G_b[j, p] + G_a[p, p] G_b[p, p] / 2 )
    info_mean[k, l] += sum_{p in M} u_p[k] u_p[l],     u_p = Z[p, :] X[S, :]

both times r.  Built per block from the plan of group_reference.plan -- by the two triangular products on the whole block,
not by the members' solves and the truncated substitutions the kernel runs."""
from __future__ import annotations

import numpy as np

import fisher_reference as FR
import group_reference as GRP


def info_blocks(Sigma, Sa, pl, r=1, X=None):
    """(info, info_mean or None) over the blocks of the plan `pl`"""
    Sigma, Sa = np.asarray(Sigma, dtype=np.float64), np.asarray(Sa, dtype=np.float64)
    nd = Sa.shape[0]
    info = np.zeros((nd, nd))
    info_mean = None if X is None else np.zeros((X.shape[1], X.shape[1]))
    for b in range(pl["blocks"]):
        idx = np.asarray(pl["rows"][pl["off"][b]:pl["off"][b + 1]], dtype=np.int64)
        k = idx.size
        mem = np.array([(int(pl["mask"][b]) >> q) & 1 for q in range(k)], dtype=np.float64)
        L = np.linalg.cholesky(Sigma[np.ix_(idx, idx)])
        Z = np.linalg.solve(L, np.eye(k))
        G = Z[None] @ Sa[:, idx[:, None], idx[None, :]] @ Z.T[None]          # nd x k x k
        w = np.triu(np.ones((k, k)), 1) + 0.5 * np.eye(k)                    # [j < p] + [j == p] / 2
        info += np.einsum("ajp,bjp,jp,p->ab", G, G, w, mem)
        if X is not None:
            u = (Z @ np.asarray(X, dtype=np.float64)[idx]) * mem[:, None]    # (Z is lower triangular: row p ends at p)
            info_mean += u.T @ u
    return r * info, (None if X is None else r * info_mean)


def statement(T, locs, X, smooth_limits, dirs, nn, group, r=1):
    """(info, info_mean) of cocons_fisher_vecchia_grouped for the partition `group` of the table `nn` (the caller's, or the
    expanded one: both have the same plan)"""
    S, Sa = FR.sigma_and_directions(T, locs, X, smooth_limits, dirs)
    return info_blocks(S, Sa, GRP.plan(nn, group), r, np.asarray(X, dtype=float))
