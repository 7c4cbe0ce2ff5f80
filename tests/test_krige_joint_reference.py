"""The three CPU routes to the predictive covariance and the conditional draws (krige_joint_reference.py) agree on the
oracle's matrices, and the pinned failing request fails where the device test expects it to.

n = 1000, m = 300, inputs as test_gpu_krige._setup builds them (theta_full(scale0 = log 0.2), nugget 1e-2).  Measured:
covariance route to route 3.3e-15 of max diag Sigma_uu (bound 1e-13), draws 4.0e-14 of max |draw| (bound 1e-11); smallest
eigenvalue of the predictive covariance 0.0100 (the nugget), cond(Sigma) 1.4e4.  The draws' spread over the covariance's is
the amplification of a perturbation of the covariance by its Cholesky factorisation, about 50 here: the device test's bound
on the draws (1e-10) is the project's 1e-12 between two sum orders of the solve times that."""
import numpy as np
import pytest

import krige_joint_reference as ref
from test_gpu_krige import _setup


@pytest.fixture(scope="module")
def problem(oracle):
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(1000, 8900, 300)
    S, C, Suu = ref.matrices(oracle, th, locs, X, lp, Xp, lp, wl.SMOOTH_LIMITS)
    E = np.random.default_rng(5).standard_normal((300, 3))
    mu = Xp @ th["mean"] + ref.stochastic(S, C, X, z, th["mean"])
    return S, C, Suu, E, mu


def test_three_routes_agree(problem):
    S, C, Suu, E, mu = problem
    r = ref.routes(S, C, Suu, E, mu)
    scale_c = np.max(np.diag(Suu))
    names = sorted(r)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            dc = np.max(np.abs(r[a][0] - r[b][0])) / scale_c
            dd = np.max(np.abs(r[a][1] - r[b][1])) / np.max(np.abs(r[b][1]))
            print("routes %s / %s: cov %.2e  draws %.2e" % (a, b, dc, dd))
            assert dc <= 1e-13, (a, b, dc)
            assert dd <= 1e-11, (a, b, dd)
    ev = np.linalg.eigvalsh(r["trsm"][0])
    print("smallest eigenvalue %.4f  cond(Sigma) %.2e" % (ev[0], np.linalg.cond(S)))
    assert ev[0] > 0.009                  # the nugget (1e-2) bounds it from below


def test_literal_route_is_the_oracles(problem, oracle):
    """The lu route restates oracle.cocoSim_cond_dense: same draws to rounding on the same inputs."""
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(1000, 8900, 300)
    S, C, Suu, E, mu = problem
    want = oracle.cocoSim_cond_dense(th, locs, lp, lp, X, Xp, wl.SMOOTH_LIMITS, z, E)
    got = ref.routes(S, C, Suu, E, mu)["lu"][1]
    assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want))


def test_failing_request_fails_at_minor_two(oracle):
    """The pinned request (n = 600): first pivot of its predictive covariance positive (measured 0.0208), second below -1
    (measured -49.3), entry [0, 1] below -1 (measured -1.013); with Sigma_uu at the prediction locations themselves it is
    positive definite."""
    from cocons_amd import workloads as wl
    locs, X, th, z, _, _ = _setup(600, 8500, 4)
    lp, lu, Xp = ref.failing_request(locs)
    S, C, Suu = ref.matrices(oracle, th, locs, X, lp, Xp, lu, wl.SMOOTH_LIMITS)
    P = ref.cov_trsm(S, C, Suu)
    d = ref.pivots(P, 2)
    print("pivots %.4f %.4f  P[0,1] %.4f" % (d[0], d[1], P[0, 1]))
    assert d[0] > 0 and d[1] < -1 and P[0, 1] < -1
    S, C, Suu = ref.matrices(oracle, th, locs, X, lp, Xp, lp, wl.SMOOTH_LIMITS)
    assert np.linalg.eigvalsh(ref.cov_trsm(S, C, Suu))[0] > 0
