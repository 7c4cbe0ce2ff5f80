"""The numpy statement of cross-validated kriging (tests/cv_reference.py) without a GPU: the brute-force route (one solve
with Sigma_AA per fold) against the route through K = Sigma^-1 that the library takes, on the CPU oracle's covariance; the
2-fold case against the oracle's own kriging; the scores against closed forms and the CRPS definition; the taper's
leave-one-out statement on the dense S = T o C."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
import grad_taper_reference as GT  # noqa: E402
from test_fisher_reference import _setup  # noqa: E402

from cocons_amd import host, workloads as wl  # noqa: E402
from oracle import oracle as O  # noqa: E402

MEAN = np.array([0.3, -0.15, 0.2])


@functools.lru_cache(maxsize=None)
def problem(n):
    """the problem of test_fisher_reference._setup (coincident pair at rows 3 and 7), three realisations, the oracle's Sigma"""
    locs, X, th = _setup(n)
    th["mean"] = MEAN.copy()
    z = np.random.default_rng(500 + n).standard_normal((n, 3))
    S = O.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
    R = z - (X @ MEAN)[:, None]
    for a in (locs, X, z, S, R):
        a.setflags(write=False)
    return locs, X, th, z, S, R


@functools.lru_cache(maxsize=None)
def brute(n, layout):
    locs, X, th, z, S, R = problem(n)
    e, v = CV.cv_brute(S, R, CV.layouts(locs)[layout])
    e.setflags(write=False)
    v.setflags(write=False)
    return e, v


@pytest.mark.parametrize("n", [130, 300, 1000])
@pytest.mark.parametrize("layout", ["loo", "random10", "spatial16", "two"])
def test_k_route_equals_brute_force(n, layout):
    """gap_e, gap_v <= 1e-10 (the identity was checked at 1.8e-12 at n = 1000; with this file's brute-force route, Cholesky
    solves per fold, the worst is 1.7e-11), for
    r = 3 and for r = 1; the coincident pair (rows 3 and 7) is split over two folds in every layout."""
    locs, X, th, z, S, R = problem(n)
    lab = CV.layouts(locs)[layout]
    assert lab[3] != lab[7]
    e_ref, v_ref = brute(n, layout)
    for r in (3, 1):
        e, v = CV.cv_kroute(S, R[:, :r], lab)
        ge, gv = CV.gaps(e, v, e_ref[:, :r], v_ref)
        print("n=%d %s r=%d: gap_e %.2e gap_v %.2e (cond %.2e, var %.3g .. %.3g, smallest at %d)"
              % (n, layout, r, ge, gv, np.linalg.cond(S), v_ref.min(), v_ref.max(), int(np.argmin(v_ref))))
        assert ge <= 1e-10 and gv <= 1e-10


@pytest.mark.parametrize("n", [130, 300])
def test_two_folds_equal_the_oracles_kriging(n):
    """r = 1: resid of the 2-fold case is z_B - (systematic + stochastic) of oracle.cocoPredict_dense from A at B's sites,
    and var its sd.pred^2.  cov_rns and cov_rns_pred share the smoothness mode here (free smoothness: logistic + sqrt in
    both).  The prediction branch has no coincident-pair rule (cov_rns gives such a pair the first site's diagonal value,
    cov_rns_pred the Matern limit without the nugget), so the pair stays in one fold for this comparison."""
    locs, X, th, z, S, R = problem(n)
    lab = np.random.default_rng(5).permutation(n) % 2
    lab[7] = lab[3]
    e, v = CV.cv_kroute(S, R[:, :1], lab)
    worst_e = worst_v = 0.0
    for l in (0, 1):
        B, A = np.nonzero(lab == l)[0], np.nonzero(lab != l)[0]
        pr = O.cocoPredict_dense(th, locs[A], locs[B], X[A], X[B], wl.SMOOTH_LIMITS, z[A, 0])
        want = z[B, 0] - (pr["systematic"] + pr["stochastic"])
        worst_e = max(worst_e, float(np.max(np.abs(e[B, 0] - want) / pr["sd.pred"])))
        worst_v = max(worst_v, float(np.max(np.abs(v[B] - pr["sd.pred"] ** 2) / pr["sd.pred"] ** 2)))
    print("n=%d against cocoPredict_dense: gap_e %.2e gap_v %.2e" % (n, worst_e, worst_v))
    assert worst_e <= 1e-10 and worst_v <= 1e-10


def test_scores_closed_forms_and_definition():
    for sd in (0.3, 1.0, 2.5):
        assert abs(host.getLogScore(0.7, 0.7, sd) - (np.log(2 * np.pi) / 2 + np.log(sd))) <= 1e-15
        assert abs(host.getCRPS(0.7, 0.7, sd) - sd * (np.sqrt(2) - 1) / np.sqrt(np.pi)) <= 1e-15 * sd
    z, mu, sd = np.array([0.2, -1.3, 4.0]), np.array([0.5, 0.4, 1.0]), np.array([0.8, 0.3, 2.0])
    got = host.getCRPS(z, mu, sd)
    ls = host.getLogScore(z, mu, sd)
    from scipy.stats import norm
    assert np.max(np.abs(ls + norm.logpdf(z, mu, sd))) <= 1e-14
    for k in range(3):
        want = CV.crps_integral(z[k], mu[k], sd[k])
        print("CRPS at point %d: %.12g against the integral %.12g" % (k, got[k], want))
        assert abs(got[k] - want) <= 1e-8 * want          # (the trapezoid rule's error at 4e5 steps)


def test_taper_leave_one_out_statement():
    """the same two routes on the dense S = T o C of tests/grad_taper_reference.py, n = 150, taper range 0.25"""
    n = 150
    rng = np.random.default_rng(900 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full(scale0=np.log(0.2))
    z = rng.standard_normal((n, 2))
    S, _ = GT.taper_matrix(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, GT.wendland1_pattern(locs, 0.25))
    S = np.tril(S) + np.tril(S, -1).T                   # (the library reads the lower triangle)
    R = z - (X @ MEAN)[:, None]
    e_ref, v_ref = CV.cv_brute(S, R, np.arange(n))
    e, v = CV.cv_kroute(S, R, np.arange(n))
    ge, gv = CV.gaps(e, v, e_ref, v_ref)
    print("taper n=%d LOO: gap_e %.2e gap_v %.2e" % (n, ge, gv))
    assert ge <= 1e-10 and gv <= 1e-10
    K = np.linalg.inv(S)
    assert np.max(np.abs(v * np.diag(K) - 1)) <= 1e-10
