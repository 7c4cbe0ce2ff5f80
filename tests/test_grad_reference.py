"""The numpy / scipy statement of the analytic gradient (tests/grad_reference.py) against Richardson central differences of
the CPU oracle's objective, and the penalty / getModelLists chain rule against differences of host.getPen /
getModelLists -- all without a GPU."""
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference as GR  # noqa: E402

from cocons_amd import host, workloads as wl  # noqa: E402
from oracle import oracle as O  # noqa: E402


def _richardson(fun, x, h):
    g = np.zeros_like(x)
    for i in range(x.size):
        def d(step):
            xp, xm = x.copy(), x.copy()
            xp[i] += step
            xm[i] -= step
            return (fun(xp) - fun(xm)) / (2 * step)
        g[i] = (4 * d(h / 2) - d(h)) / 3
    return g


def _problem(n, r, seed, mean_scale=0.3):
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(n, 2))
    locs[7] = locs[3]                                # two coincident locations
    X = wl.design_from_locs(locs)["std.covs"]
    X[7] = X[3] + [0.0, 0.5, 0.5]                   # (a larger variance at the second of them: Sigma stays positive definite)
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = mean_scale * np.array([1.0, -0.5, 0.25])
    z = rng.standard_normal((n, r))
    return locs, X, th, z


def _all_free(p=3):
    pp = OrderedDict()
    for k in host.ASPECTS:
        pp[k] = [True] * p
    return pp


def test_reference_gradient_matches_oracle_differences():
    n, r = 120, 2
    locs, X, th, z = _problem(n, r, 11)
    pp = _all_free()
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.0, 0.0, 0.0)

    def fun(x):
        return O.GetNeg2loglikelihood(x, pp, locs, X, wl.SMOOTH_LIMITS, z, n, lam, safe=False)

    num = _richardson(fun, x0, 1e-4)
    tl = host.getModelLists(x0, pp, "diff")
    f, gt, gm = GR.neg2loglik_grad(host.theta_table(tl), tl["mean"], locs, X, z, wl.SMOOTH_LIMITS)
    assert abs(f - fun(x0)) <= 1e-9 * abs(f)
    g = OrderedDict(mean=gm)
    for t, k in enumerate(host.COV_ASPECTS):
        g[k] = gt[t]
    ana = host.getModelLists_grad(g, pp)
    err = np.max(np.abs(ana - num))
    assert err <= 1e-6 * np.max(np.abs(num)), (err, np.max(np.abs(num)))


def test_reference_fixed_smoothness_modes():
    n, r = 80, 1
    locs, X, th, z = _problem(n, r, 5)
    for nu in (0.5, 1.5, 2.5):
        th2 = OrderedDict((k, np.array(v, float)) for k, v in th.items())
        th2["smooth"] = np.zeros(3)
        sl = (nu, nu)
        T = host.theta_table(th2)

        def fun(t):
            tl = OrderedDict(th2)
            for i, k in enumerate(host.COV_ASPECTS):
                tl[k] = t[i]
            S = O.cov_rns(tl, locs, X, sl)
            L = np.linalg.cholesky(S)
            w = np.linalg.solve(L, z[:, 0] - X @ th2["mean"])
            return n * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(L))) + w @ w

        f, gt, gm = GR.neg2loglik_grad(T, th2["mean"], locs, X, z, sl)
        assert np.all(gt[4] == 0)
        for t in (0, 1, 2, 3, 5):
            for k in range(3):
                def fk(x, t=t, k=k):
                    TT = T.copy()
                    TT[t, k] = x[0]
                    return fun(TT)
                num = _richardson(fk, np.array([T[t, k]]), 1e-4)[0]
                assert abs(gt[t, k] - num) <= 1e-6 * max(1.0, np.max(np.abs(gt))), (nu, t, k, gt[t, k], num)


def test_penalty_and_diff_chain_rule():
    pp = wl.par_pos_full()
    th = wl.theta_full(scale0=np.log(0.2))
    th["std.dev"] = np.array([0.1, 3e-5, -0.2])       # one entry on the smooth branch of sumsmoothlone
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.7, 0.3, 0.2)
    N = 250

    def pen(x):
        return host.getPen(N, lam, host.getModelLists(x, pp, "diff"), wl.SMOOTH_LIMITS)

    tl = host.getModelLists(x0, pp, "diff")
    ana = host.getModelLists_grad(host.getPen_grad(N, lam, tl, wl.SMOOTH_LIMITS), pp)
    num = np.zeros_like(x0)
    for i in range(x0.size):
        xp, xm = x0.copy(), x0.copy()
        step = 1e-7                                     # (small against 1 / alpha's scale of the smooth branch)
        xp[i] += step
        xm[i] -= step
        num[i] = (pen(xp) - pen(xm)) / (2 * step)
    assert np.max(np.abs(ana - num)) <= 1e-6 * np.max(np.abs(num)), (ana, num)
