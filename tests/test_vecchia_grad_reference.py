"""The numpy statement of the Vecchia gradient (tests/vecchia_grad_reference.py) without a GPU: against central differences of
vecchia_reference's values on the oracle's Sigma, against the dense gradient where the table makes the approximation exact,
its Profile and REML compositions against differences of profile_value / reml_value -- and the new entry at the boundary
(declared, bound, exported, bad calls refused before any device work)."""
import ctypes
import os
import re
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference as GR  # noqa: E402
import vecchia_grad_reference as VG  # noqa: E402
import vecchia_reference as VR  # noqa: E402

from cocons_amd import host, workloads as wl  # noqa: E402
from oracle import oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    X[7] = X[3] + [0.0, 0.5, 0.5]                   # (a larger variance at the second of them: the blocks stay positive definite)
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = mean_scale * np.array([1.0, -0.5, 0.25])
    z = rng.standard_normal((n, r))
    return locs, X, th, z


def _free(mean=True, p=3):
    pp = OrderedDict()
    for k in host.ASPECTS:
        pp[k] = [mean or k != "mean"] * p
    return pp


def _vector_grad(gt, gm, pp, p=3):
    g = OrderedDict(mean=np.zeros(p) if gm is None else gm)
    for t, k in enumerate(host.COV_ASPECTS):
        g[k] = gt[t]
    return host.getModelLists_grad(g, pp)


def test_statement_matches_differences_of_the_vecchia_value():
    n, r, m = 100, 2, 10
    locs, X, th, z = _problem(n, r, 11)
    nn = host.vecchia_neighbours(locs, m)
    pp = _free()
    x0 = wl.theta_vector_from_lists(th, pp)

    def fun(x):
        tl = host.getModelLists(x, pp, "diff")
        S = O.cov_rns(tl, locs, X, wl.SMOOTH_LIMITS)
        return VR.neg2loglik(S, nn, z - (X @ tl["mean"])[:, None])[0]

    num = _richardson(fun, x0, 1e-4)
    tl = host.getModelLists(x0, pp, "diff")
    S = O.cov_rns(tl, locs, X, wl.SMOOTH_LIMITS)
    own, _ = VG.sigma_and_contract(host.theta_table(tl), locs, X, wl.SMOOTH_LIMITS, [])
    assert np.max(np.abs(own - S)) <= 1e-12 * np.max(np.abs(S))
    f, parts, gt, gq, gm = VG.neg2loglik_grad(host.theta_table(tl), tl["mean"], locs, X, z, wl.SMOOTH_LIMITS, nn, Sigma=S)
    assert abs(f - fun(x0)) <= 1e-12 * abs(f)
    ana = _vector_grad(gt, gm, pp)
    err = np.max(np.abs(ana - num))
    print("vecchia statement vs differences: err %.3e of %.3e" % (err, np.max(np.abs(num))))
    assert err <= 1e-6 * np.max(np.abs(num)), (err, np.max(np.abs(num)))
    # the quadratic forms' share alone: differences of the sum of squares of the whitened columns
    ppc = _free(mean=False)
    xc = wl.theta_vector_from_lists(th, ppc)

    def quad(x):
        S = O.cov_rns(host.getModelLists(x, ppc, "diff"), locs, X, wl.SMOOTH_LIMITS)
        return float(np.sum(VR.neg2loglik(S, nn, z - (X @ th["mean"])[:, None])[1][1:]))

    numq = _richardson(quad, xc, 1e-4)
    anaq = _vector_grad(gq, None, ppc)
    assert np.max(np.abs(anaq - numq)) <= 1e-6 * np.max(np.abs(numq)), (anaq, numq)


# measured: 3.5e-15 of the largest entry of the dense gradient (n = 60, r = 2); asserted at ten times that
EXACT_GAP = 3.5e-14


def test_all_predecessors_gives_the_dense_gradient():
    n, r = 60, 2
    locs, X, th, z = _problem(n, r, 3)
    T = host.theta_table(th)
    f, gt, gm = GR.neg2loglik_grad(T, th["mean"], locs, X, z, wl.SMOOTH_LIMITS)
    fv, _, vt, _, vm = VG.neg2loglik_grad(T, th["mean"], locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    scale = max(np.max(np.abs(gt)), np.max(np.abs(gm)))
    gap = max(np.max(np.abs(vt - gt)), np.max(np.abs(vm - gm))) / scale
    print("all predecessors vs dense gradient: gap %.3e" % gap)
    assert abs(fv - f) <= 1e-12 * abs(f)
    assert gap <= EXACT_GAP, gap


def test_a_short_table_moves_the_gradient():
    n, r, m = 300, 1, 10
    locs, X, th, z = _problem(n, r, 5)
    T = host.theta_table(th)
    _, gt, gm = GR.neg2loglik_grad(T, th["mean"], locs, X, z, wl.SMOOTH_LIMITS)
    _, _, vt, _, vm = VG.neg2loglik_grad(T, th["mean"], locs, X, z, wl.SMOOTH_LIMITS, host.vecchia_neighbours(locs, m))
    gap = np.max(np.abs(vt - gt)) / np.max(np.abs(gt))
    print("m = 10 against the dense gradient: gap %.3e" % gap)
    assert gap > 1e-4, gap                          # (every tolerance here is 1e-6 or tighter)


def test_profile_and_reml_compositions_match_differences():
    n, r, m = 90, 2, 8
    locs, X, th, z = _problem(n, r, 17)
    z = z + (X @ np.array([0.8, -0.4, 0.3]))[:, None]
    nn = host.vecchia_neighbours(locs, m)
    pp = _free(mean=False)
    x0 = wl.theta_vector_from_lists(th, pp)

    def sigma(x):
        return O.cov_rns(host.getModelLists(x, pp, "diff"), locs, X, wl.SMOOTH_LIMITS)

    T = host.theta_table(host.getModelLists(x0, pp, "diff"))
    for name, value, ana in (
            ("profile", lambda x: VR.profile_value(sigma(x), nn, z, X), VG.profile_grad(T, locs, X, z, X, wl.SMOOTH_LIMITS, nn)),
            ("reml", lambda x: VR.reml_value(sigma(x), nn, z, X), VG.reml_grad(T, locs, X, z, wl.SMOOTH_LIMITS, nn))):
        num = _richardson(value, x0, 1e-4)
        val, gt = ana
        assert abs(val - value(x0)) <= 1e-10 * abs(val), (name, val, value(x0))
        got = _vector_grad(gt, None, pp)
        err = np.max(np.abs(got - num))
        print("%s composition vs differences: err %.3e of %.3e" % (name, err, np.max(np.abs(num))))
        assert err <= 1e-6 * np.max(np.abs(num)), (name, err)


# ---- the entry at the boundary (fails on a library without it) ------------------------------------------------------------
DECL = (r"int\s+cocons_neg2loglik_grad_vecchia\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
        r"int c,\s*const double \*B,\s*double \*sum_logliks,\s*double \*parts,\s*double \*grad_theta,\s*double \*grad_quad,\s*"
        r"double \*grad_mean\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_entry_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    name = "cocons_neg2loglik_grad_vecchia"
    assert re.search(DECL, open(os.path.join(ROOT, "include", "cocons_hip.h")).read())
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 10
    assert hasattr(L, name)
    for fn in ("GetNeg2loglikelihoodVecchia_grad", "GetNeg2loglikelihoodVecchiaProfile_grad",
               "GetNeg2loglikelihoodVecchiaREML_grad"):
        assert callable(getattr(host, fn))
    assert hasattr(host.CoconsVecchiaFit, "neg2loglik_grad_core")


def test_entry_refuses_bad_calls_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    fn, who = L.cocons_neg2loglik_grad_vecchia, "cocons_neg2loglik_grad_vecchia"
    p = 3
    th, mean, B = np.zeros(6 * p), np.zeros(p), np.zeros(8)
    val = ctypes.c_double(7.0)
    parts, gt, gq, gm = np.full(6, 7.0), np.full(6 * p, 7.0), np.full(6 * p, 7.0), np.full(p, 7.0)
    v = ctypes.byref(val)
    assert fn(None, _dp(th), _dp(mean), 0, None, v, _dp(parts), _dp(gt), _dp(gq), _dp(gm)) == -1
    msg = _lib.last_error()
    assert msg.startswith(who + ":") and "null fit handle" in msg, msg
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the arguments are checked first
    for args in ((None, _dp(mean), 0, None, v, _dp(parts), _dp(gt), _dp(gq), _dp(gm)),
                 (_dp(th), None, 0, None, v, _dp(parts), _dp(gt), _dp(gq), _dp(gm)),
                 (_dp(th), _dp(mean), 0, None, None, _dp(parts), _dp(gt), _dp(gq), _dp(gm)),
                 (_dp(th), _dp(mean), 0, None, v, _dp(parts), None, _dp(gq), _dp(gm)),
                 (_dp(th), _dp(mean), 0, None, v, _dp(parts), _dp(gt), _dp(gq), None),
                 (_dp(th), None, 1, _dp(B), v, _dp(parts), None, _dp(gq), None)):
        assert fn(bogus, *args) == -1
        assert _lib.last_error().startswith(who + ": null argument"), _lib.last_error()
    # B together with mean or grad_mean, and c < 1
    for args in ((_dp(th), _dp(mean), 1, _dp(B), v, _dp(parts), _dp(gt), _dp(gq), None),
                 (_dp(th), None, 1, _dp(B), v, _dp(parts), _dp(gt), _dp(gq), _dp(gm))):
        assert fn(bogus, *args) == -1
        msg = _lib.last_error()
        assert msg.startswith(who + ": B is given") and "must be NULL" in msg, msg
    assert fn(bogus, _dp(th), None, 0, _dp(B), v, _dp(parts), _dp(gt), _dp(gq), None) == -1
    assert _lib.last_error().startswith(who + ": c = 0"), _lib.last_error()
    assert val.value == 7.0 and all(np.all(a == 7.0) for a in (parts, gt, gq, gm))
