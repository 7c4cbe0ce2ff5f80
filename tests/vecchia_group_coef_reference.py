"""Numpy block form of the grouped Vecchia coefficients (launch_vecchia_group_coefs; test infrastructure, not
a test module): one Cholesky factor per block of group_reference.plan, then one backward solve per member on the leading
sub-factor, scattered into the n x (m + 1) layout of vecchia_sim_reference.coefficients.

For a block with rows S ascending and K = L L' on them, the member at position p has s_p = L_{0..p}^-T e_p, component j
= (e_p[j] - sum_{i > j} L(i, j) s_p[i]) / L(j, j).  The row's stored neighbours are the block's positions 0 .. p - 1 (the table
is closed under the partition), so places t < p hold s_p[t], places p .. m - 1 hold 0 and place m holds s_p[p]."""
import numpy as np

import group_reference as GR


def coefficients(S, wide, group, n_fixed=0, m_out=None, fill=0.0):
    """n x (m_out + 1) float64 (m_out None: the table's width): the records of the member rows >= n_fixed; the rows below
    n_fixed keep `fill` in every place -- nothing is written for them"""
    S, wide = np.asarray(S, dtype=np.float64), np.asarray(wide)
    n = wide.shape[0]
    m = wide.shape[1] if m_out is None else int(m_out)
    pl = GR.plan(wide, group)
    if m < pl["longest"]:
        raise ValueError("m_out = %d is smaller than the longest expanded row (%d)" % (m, pl["longest"]))
    out = np.full((n, m + 1), fill, dtype=np.float64)
    for b in range(pl["blocks"]):
        rows = pl["rows"][pl["off"][b]:pl["off"][b + 1]]
        if rows[-1] < n_fixed:
            continue                                    # every row of the block is fixed
        L = np.linalg.cholesky(S[np.ix_(rows, rows)])    # ONE factor for the block
        for p, row in enumerate(rows):
            if not (pl["mask"][b] >> p) & 1 or row < n_fixed:
                continue
            s = np.zeros(p + 1)
            for j in range(p, -1, -1):                   # L_{0..p}' s = e_p, backwards
                s[j] = ((1.0 if j == p else 0.0) - np.sum(L[j + 1:p + 1, j] * s[j + 1:])) / L[j, j]
            out[row] = 0.0
            out[row, :p] = s[:p]
            out[row, m] = s[p]
    return out
