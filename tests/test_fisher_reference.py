"""The numpy / scipy statement of the expected information (tests/fisher_reference.py) without a GPU: its derivative
matrices against Richardson differences of the CPU oracle's covariance, its two forms against each other, the exact scaling
identity I(v_s, v_s) = r n / 2, and the host's Jacobian assembly (host.fisher_to_par) against getModelLists_grad."""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402

from cocons_amd import host, workloads as wl  # noqa: E402
from oracle import oracle as O  # noqa: E402

N = 300


def _setup(n, seed=3):
    """the problem of test_gpu_grad._setup with the coincident pair"""
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(n, 2))
    locs[7] = locs[3]
    X = wl.design_from_locs(locs)["std.covs"]
    X[7] = X[3] + [0.0, 0.5, 0.5]
    th = wl.theta_full(scale0=np.log(0.2))
    return locs, X, th


@functools.lru_cache(maxsize=None)
def _reference():
    locs, X, th = _setup(N)
    S, dS = FR.sigma_and_partials(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS)
    for a in (S, dS):
        a.setflags(write=False)
    return locs, X, th, S, dS


def test_derivative_matrices_match_oracle_differences():
    locs, X, th, S, dS = _reference()
    So = O.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
    gap = np.max(np.abs(S - So)) / np.max(np.abs(So))
    print("Sigma against the oracle: %.2e" % gap)
    assert gap <= 1e-12
    h = 1e-4
    worst = 0.0
    for t, name in enumerate(host.COV_ASPECTS):
        for k in range(3):
            def cov(step):
                tl = OrderedDict((kk, np.array(v, float)) for kk, v in th.items())
                tl[name][k] += step
                return O.cov_rns(tl, locs, X, wl.SMOOTH_LIMITS)
            d1 = (cov(h) - cov(-h)) / (2 * h)
            d2 = (cov(h / 2) - cov(-h / 2)) / h
            num = (4 * d2 - d1) / 3
            err = np.max(np.abs(dS[t, k] - num)) / max(np.max(np.abs(num)), 1e-300)
            worst = max(worst, err)
            assert err <= 1e-6, (name, k, err)
    print("derivative matrices against Richardson differences of the oracle: worst %.2e of the largest entry" % worst)


def test_two_forms_agree_and_scaling_identity():
    locs, X, th, S, dS = _reference()
    dirs = np.concatenate([np.eye(18).reshape(18, 6, 3), FR.scaling_direction(3)[None]])
    Sa = FR.direction_matrices(dS, dirs)
    assert np.max(np.abs(Sa[18] - S)) <= 1e-13 * np.max(np.abs(S))          # Sigma_v = Sigma
    S2, Sa2 = FR.sigma_and_directions(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, dirs)   # (the route without the 6 p matrices)
    assert np.array_equal(S2, S) and np.max(np.abs(Sa2 - Sa)) <= 1e-13 * np.max(np.abs(Sa))
    for r in (1, 3):
        I1, I2 = FR.info_solve(S, Sa, r), FR.info_whiten(S, Sa, r)
        gap = FR.metric(I1, I2)
        print("r=%d the two forms: %.2e; I(v_s, v_s) - r n / 2 = %.2e; diagonal %.3g .. %.3g; smallest eigenvalue %.3g"
              % (r, gap, I1[18, 18] - r * N / 2, np.min(np.diag(I1)[:18]), np.max(np.diag(I1)[:18]),
                 np.linalg.eigvalsh(I1[:18, :18])[0]))
        assert gap <= 1e-12
        for I in (I1, I2):
            assert abs(I[18, 18] - r * N / 2) <= 1e-12 * N
        assert np.linalg.eigvalsh(I1[:18, :18])[0] > 0


def test_host_chain_rule():
    """J_t I J_t' + J_m I_m J_m' (host.fisher_to_par) is getModelLists_grad applied to the columns, then to the rows."""
    pp = wl.par_pos_full()
    pp["mean"] = [True] * 3
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = np.array([0.3, -0.15, 0.2])
    x0 = wl.theta_vector_from_lists(th, pp)
    rng = np.random.default_rng(17)
    A = rng.standard_normal((18, 18))
    It = A @ A.T
    B = rng.standard_normal((3, 3))
    Im = B @ B.T
    full = np.zeros((21, 21))                       # (mean, table) x (mean, table): the block between them is 0
    full[:3, :3] = Im
    full[3:, 3:] = It

    def chain(vec21):
        g = OrderedDict(mean=vec21[:3])
        for t, k in enumerate(host.COV_ASPECTS):
            g[k] = vec21[3 + 3 * t:6 + 3 * t]
        return host.getModelLists_grad(g, pp)

    half = np.stack([chain(full[:, j]) for j in range(21)], axis=1)         # P x 21
    want = np.stack([chain(half[i]) for i in range(half.shape[0])], axis=0)  # P x P
    got = host.fisher_to_par(It, Im, x0, pp)
    assert got.shape == (x0.size, x0.size) == (19, 19)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    assert np.array_equal(got, got.T) or np.max(np.abs(got - got.T)) <= 1e-13 * np.max(np.abs(got))
    Jt, Jm = host.fisher_jacobian(x0, pp)
    assert np.all(Jt[:3] == 0) and np.all(Jm[3:] == 0)                      # mean parameters first, as par_pos orders them
