"""What the tests of the Vecchia neighbours by model correlation share: the brute-force statement of the rule of
include/cocons_hip.h -- per row build the set of candidates, sort it by the key, take m --, the point sets and covariances of the
cases, the thetas, and the KL divergence of a Vecchia model from the exact one.

The rule: N(i) is row i of the Euclidean ordered table of width m_cand; C(i) = N(i) for hops = 1, N(i) and the N(j) of its
members j for hops = 2, zeros dropped, each index once; key (rho descending, index ascending) with
rho = fl(S[j, i] / fl(sqrt(fl(S[i, i] S[j, j])))) compared by the total order of its bit patterns; row i lists the m candidates with
the largest key, 1-based, zero-padded."""
import math
import struct

import numpy as np

import knn_reference as KR

SETTINGS = ((60, 1), (30, 2), (60, 2))          # (m_cand, hops) of the tool and the report, at m = 30


def _ordered_bits(rho):
    b = struct.unpack("<Q", struct.pack("<d", rho))[0]
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def brute(S, nn_cand, m, hops):
    """the rule, row by row, with Python sets, floats and a sort"""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    cand = np.asarray(nn_cand).reshape(n, -1)
    out = np.zeros((n, m), dtype=np.int32, order="F")
    for i in range(n):
        near = [int(v) - 1 for v in cand[i] if v > 0]
        C = set(near)
        if hops == 2:
            for j in near:
                C.update(int(v) - 1 for v in cand[j] if v > 0)
        assert all(j < i for j in C)
        keyed = []
        for j in C:
            rho = float(S[j, i]) / math.sqrt(float(S[i, i]) * float(S[j, j]))
            assert math.isfinite(rho)
            keyed.append((-_ordered_bits(rho), j))
        keyed.sort()
        for k, (_, j) in enumerate(keyed[:m]):
            out[i, k] = j + 1
    return out


def scaled(m_cand, m):
    """a setting of the report (stated at m = 30) at another m: m_cand in the same proportion"""
    return m_cand * m // 30


# ---- point sets and covariances of the rule's cases (plain numpy: the rule does not care where S comes from) ----------------
def aniso_exp(locs, ratio=4.0, rng_=0.3, nugget=0.01):
    """exp(-d_A) + nugget I with the x axis `ratio` times as long as the y axis"""
    dx = (locs[:, None, 0] - locs[None, :, 0]) / (rng_ * ratio)
    dy = (locs[:, None, 1] - locs[None, :, 1]) / rng_
    return np.exp(-np.sqrt(dx * dx + dy * dy)) + nugget * np.eye(locs.shape[0])


def lattice_ties(nx=12, ny=12, seed=3):
    """an integer lattice in a shuffled order with S a function of the exact integer d2 alone: rho ties exactly, in rings"""
    locs = KR.lattice(nx, ny)[np.random.default_rng(seed).permutation(nx * ny)]
    d2 = (locs[:, None, 0] - locs[None, :, 0]) ** 2 + (locs[:, None, 1] - locs[None, :, 1]) ** 2
    return locs, np.exp(-0.25 * np.sqrt(d2)) + 0.5 * np.eye(nx * ny)


def coincident(n=90, seed=5):
    """every site three times over, shuffled: predecessors at distance 0"""
    rng = np.random.default_rng(seed)
    locs = np.repeat(rng.uniform(0, 1, size=(n // 3, 2)), 3, axis=0)[rng.permutation(n)]
    return locs, aniso_exp(locs, nugget=0.05)


# ---- the thetas of tools/vecchia_corr_kl.py and of the KL condition --------------------------------------------------------
def theta_iso():
    """the stationary isotropic setting of tools/vecchia_order_kl.py, intercept only"""
    return {"mean": np.zeros(1), "std.dev": np.zeros(1), "scale": np.array([np.log(0.15)]), "aniso": np.zeros(1),
            "tilt": np.zeros(1), "smooth": np.zeros(1), "nugget": np.array([np.log(1e-8)])}


def theta_aniso(ratio=5.0, nugget=1e-2):
    """the same with a global geometric anisotropy: the kernel matrix is rd diag(1, an^2), an = exp(aniso) = the ratio of
    its axes' lengths (tilt 0 is an angle of pi / 2: no rotation)"""
    th = theta_iso()
    th["aniso"] = np.array([np.log(ratio)])
    th["nugget"] = np.array([np.log(nugget)])
    return th


def theta_covariate(nugget=1e-2):
    """anisotropy, tilt and range driven by the covariates [1, x, y] (workloads.design_from_locs)"""
    return {"mean": np.zeros(3), "std.dev": np.array([0.0, 0.2, -0.1]), "scale": np.array([np.log(0.15), 0.3, 0.2]),
            "aniso": np.array([np.log(3.0), 0.6, -0.6]), "tilt": np.array([0.0, 0.8, 0.5]), "smooth": np.array([0.0, 0.3, -0.3]),
            "nugget": np.array([np.log(nugget), 0.0, 0.0])}


def kl(S, nn, half_logdet=None):
    """KL of the Vecchia model of the table nn from the exact one: sum_i log d_i - 1/2 log det Sigma"""
    import vecchia_reference as VR
    if half_logdet is None:
        half_logdet = float(np.sum(np.log(np.diag(np.linalg.cholesky(S)))))
    return float(np.sum(VR.whiten(S, nn, np.zeros((S.shape[0], 1)))[1])) - half_logdet
