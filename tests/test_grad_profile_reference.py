"""The numpy statement of the Profile / REML gradients (tests/grad_profile_reference.py) against Richardson central
differences of the CPU oracle's GetNeg2loglikelihoodProfile / ...REML (all six covariance aspects free, the mean fixed; Profile
with q = 2 != p = 3 columns, one coincident pair), and the host penalty path of REML's N = (n - rank) r against differences of
host.getPen -- all without a GPU.  Tolerance 1e-6 of the largest gradient entry, as tests/test_grad_reference.py
(measured: 1.4e-10 for both objectives)."""
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_profile_reference as GPR  # noqa: E402
from test_grad_reference import _problem, _richardson  # noqa: E402

from cocons_amd import host, workloads as wl  # noqa: E402
from oracle import oracle as O  # noqa: E402


def _cov_free(p=3):
    pp = OrderedDict()
    pp["mean"] = [False] * p
    for k in host.COV_ASPECTS:
        pp[k] = [True] * p
    return pp


def _check(fun, x0, pp, gt, f):
    num = _richardson(fun, x0, 1e-4)
    assert abs(f - fun(x0)) <= 1e-9 * abs(f)
    g = OrderedDict(mean=np.zeros(3))
    for t, k in enumerate(host.COV_ASPECTS):
        g[k] = gt[t]
    ana = host.getModelLists_grad(g, pp)
    err = np.max(np.abs(ana - num))
    print("max error %.3e of %.3e" % (err, np.max(np.abs(num))))
    assert err <= 1e-6 * np.max(np.abs(num)), (err, np.max(np.abs(num)))


def test_profile_reference_gradient_matches_oracle_differences():
    n, r = 120, 2
    locs, X, th, z = _problem(n, r, 11)
    xb = X[:, :2].copy()
    pp = _cov_free()
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.0, 0.0, 0.0)
    tl = host.getModelLists(x0, pp, "diff")
    f, gt, _, _ = GPR.profile_grad(tl, locs, X, z, xb, wl.SMOOTH_LIMITS)
    _check(lambda x: O.GetNeg2loglikelihoodProfile(x, pp, locs, X, wl.SMOOTH_LIMITS, z, n, xb, lam, safe=False), x0, pp, gt, f)


def test_reml_reference_gradient_matches_oracle_differences():
    n, r = 120, 2
    locs, X, th, z = _problem(n, r, 11)
    pp = _cov_free()
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.0, 0.0, 0.0)
    tl = host.getModelLists(x0, pp, "diff")
    f, gt, _, _ = GPR.reml_grad(tl, locs, X, z, wl.SMOOTH_LIMITS)
    _check(lambda x: O.GetNeg2loglikelihoodREML(x, pp, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, safe=False), x0, pp, gt, f)


def test_reml_penalty_path():
    """getPen_grad with REML's N = (n - rank) r through getModelLists_grad, against differences of host.getPen."""
    pp = _cov_free()
    th = wl.theta_full(scale0=np.log(0.2))
    th["aniso"] = np.array([0.1, 3e-5, -0.2])         # one entry on the smooth branch of sumsmoothlone
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.7, 0.3, 0.2)
    n, rank, r = 120, 3, 2
    N = (n - rank) * r

    def pen(x):
        return host.getPen(N, lam, host.getModelLists(x, pp, "diff"), wl.SMOOTH_LIMITS)

    tl = host.getModelLists(x0, pp, "diff")
    ana = host.getModelLists_grad(host.getPen_grad(N, lam, tl, wl.SMOOTH_LIMITS), pp)
    num = np.zeros_like(x0)
    for i in range(x0.size):
        xp, xm = x0.copy(), x0.copy()
        xp[i] += 1e-7
        xm[i] -= 1e-7
        num[i] = (pen(xp) - pen(xm)) / 2e-7
    assert ana.shape == x0.shape
    assert np.max(np.abs(ana - num)) <= 1e-6 * np.max(np.abs(num)), (ana, num)
