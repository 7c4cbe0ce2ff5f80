"""What the tests of the neighbours of NEW locations by model correlation share: the brute-force statement of the
rule of include/cocons_hip.h -- per new location build the set of candidates, sort it by the key, take m --, numpy
cross-covariances of the rule's cases, and the excess of a local-kriging variance over the exact one.

The rule: P(q) is the plain kNN of q among all observations, width m_cand; C(q) = P(q) for hops = 1, P(q) and the plain kNN
A(j) of every member j's own coordinates for hops = 2, zeros dropped, each index once; key (rho descending, index ascending)
with rho = fl(Cq[q, j] / fl(sqrt(fl(dq[q] d[j])))) compared by the total order of its bit patterns; row q lists the m
candidates with the largest key, 1-based, zero-padded."""
import math

import numpy as np

from corr_knn_reference import _ordered_bits

SETTINGS = ((60, 1), (30, 2), (60, 2))          # (m_cand, hops) of the tool and the report, at m = 30


def brute(Cq, dq, d, nn_pred, nn_all, m, hops):
    """the rule, row by row, with Python sets, floats and a sort"""
    Cq = np.asarray(Cq, dtype=np.float64)
    mp, n = Cq.shape
    first = np.asarray(nn_pred).reshape(mp, -1)
    lists = np.asarray(nn_all).reshape(n, -1)
    out = np.zeros((mp, m), dtype=np.int32, order="F")
    for q in range(mp):
        near = [int(v) - 1 for v in first[q] if v > 0]
        C = set(near)
        if hops == 2:
            for j in near:
                C.update(int(v) - 1 for v in lists[j] if v > 0)
        keyed = []
        for j in C:
            rho = float(Cq[q, j]) / math.sqrt(float(dq[q]) * float(d[j]))
            assert math.isfinite(rho)
            keyed.append((-_ordered_bits(rho), j))
        keyed.sort()
        for k, (_, j) in enumerate(keyed[:m]):
            out[q, k] = j + 1
    return out


def aniso_cross(locs, q, ratio=4.0, rng_=0.3, nugget=0.01):
    """(Cq, dq, d) of corr_knn_reference.aniso_exp for new sites q: exp(-d_A) off the sites, and at an exact coordinate match
    the new site's diagonal value 1 + nugget (the prediction entry's rule)"""
    dx = (q[:, None, 0] - locs[None, :, 0]) / (rng_ * ratio)
    dy = (q[:, None, 1] - locs[None, :, 1]) / rng_
    Cq = np.exp(-np.sqrt(dx * dx + dy * dy))
    match = (q[:, None, 0] == locs[None, :, 0]) & (q[:, None, 1] == locs[None, :, 1])
    Cq[match] = 1.0 + nugget
    return Cq, np.full(q.shape[0], 1.0 + nugget), np.full(locs.shape[0], 1.0 + nugget)


def lattice_cross(locs, q):
    """the same for corr_knn_reference.lattice_ties: a function of the exact integer (or half-integer) d2 alone"""
    d2 = (q[:, None, 0] - locs[None, :, 0]) ** 2 + (q[:, None, 1] - locs[None, :, 1]) ** 2
    Cq = np.exp(-0.25 * np.sqrt(d2))
    Cq[d2 == 0] = 1.5
    return Cq, np.full(q.shape[0], 1.5), np.full(locs.shape[0], 1.5)


def excess_variance(S, Cp, dq, nn):
    """(mean, worst) of (local-kriging variance of the table nn) / (exact kriging variance) - 1 over the new sites: S the
    observations' covariance, Cp the cross-covariance (mp x n), dq the new sites' variances.  The exact variance conditions
    on every observation, so no table can go below it."""
    L = np.linalg.cholesky(S)
    V = np.linalg.solve(L, Cp.T)
    exact = dq - np.sum(V * V, axis=0)
    local = np.empty_like(exact)
    for q in range(Cp.shape[0]):
        idx = nn[q][nn[q] > 0] - 1
        c = Cp[q, idx]
        local[q] = dq[q] - c @ np.linalg.solve(S[np.ix_(idx, idx)], c)
    ex = local / exact - 1.0
    return float(ex.mean()), float(ex.max())
