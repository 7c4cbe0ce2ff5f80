"""cocons_cv_dense on the GPU -- cross-validated predictions from one factorisation -- against the numpy statement of
tests/cv_reference.py on the CPU oracle's covariance: brute force per fold (one Cholesky of Sigma_AA each) wherever that is
cheap, the K-route for leave-one-out at n = 2116 (tests/test_cv_reference.py pins the two to each other at 1e-10).

The bound of every comparison is the project's parity bound for values, 1e-8, in
    gap_e = max |resid - resid_ref| / sd_ref      and      gap_v = max |var - var_ref| / var_ref.
Every case prints its gaps before it asserts."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
from test_fisher_reference import _setup as _coincident_setup  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 1e-8
MEAN = np.array([0.3, -0.15, 0.2])


@functools.lru_cache(maxsize=None)
def problem(n, nu=None):
    """the problem of test_fisher_reference._setup (coincident pair at rows 3 and 7) with three realisations and the oracle's
    Sigma; nu: fixed smoothness (smooth.limits = (nu, nu), zero smooth vector)"""
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    locs, X, th = _coincident_setup(n)
    th["mean"] = MEAN.copy()
    sl = tuple(wl.SMOOTH_LIMITS)
    if nu is not None:
        th["smooth"] = np.zeros(3)
        sl = (nu, nu)
    z = np.random.default_rng(500 + n).standard_normal((n, 3))
    S = O.cov_rns(th, locs, X, sl)
    R = z - (X @ MEAN)[:, None]
    for a in (locs, X, z, S, R):
        a.setflags(write=False)
    return locs, X, th, z, S, R, sl


@functools.lru_cache(maxsize=None)
def reference(n, layout, nu=None):
    """(labels, resid n x 3, var) -- computed once, shared, read-only"""
    locs, X, th, z, S, R, sl = problem(n, nu)
    lab = labels(n, layout)
    e, v = (CV.cv_kroute if (layout == "loo" and n > 1000) else CV.cv_brute)(S, R, lab)
    for a in (lab, e, v):
        a.setflags(write=False)
    return lab, e, v


def labels(n, layout):
    locs = problem(n)[0]
    if layout in ("loo", "random10", "spatial16", "two"):
        return CV.layouts(locs)[layout]
    if layout == "mixed":       # n = 700: folds of 1, 2, 16, 17, 127, 128, 129 and the rest (every regime and every boundary)
        sizes = [1, 2, 16, 17, 127, 128, 129]
        sizes.append(n - sum(sizes))
        lab = np.repeat(np.arange(len(sizes)), sizes)
        return CV._apart(np.random.default_rng(23).permutation(lab), 3, 7)
    raise KeyError(layout)


def fit_for(n, r, nu=None):
    import cocons_amd as ca
    locs, X, th, z, S, R, sl = problem(n, nu)
    return ca.CoconsFit(locs, X, z[:, :r], sl), th


def check(tag, got, n, layout, r, nu=None):
    lab, e, v = reference(n, layout, nu)
    ge, gv = CV.gaps(got[0], got[1], e[:, :r], v)
    print("%s n=%d %s r=%d: gap_e %.3e gap_v %.3e (var %.3g .. %.3g)" % (tag, n, layout, r, ge, gv, v.min(), v.max()))
    assert got[0].shape == (n, r) and got[1].shape == (n,)
    assert ge <= BOUND and gv <= BOUND, (ge, gv)


@pytest.mark.parametrize("r", [1, 3])
def test_n300_every_layout(r):
    """n = 300 with the coincident pair in different folds: leave-one-out (closed form), 10 random folds of 30 and 16 spatial
    blocks (LDS kernel, classes 16 / 32 / 64), 2 folds of 150 (the library's factorisation on the call's scratch)."""
    fit, th = fit_for(300, r)
    try:
        for layout in ("loo", "random10", "spatial16", "two"):
            lab = reference(300, layout)[0]
            assert lab[3] != lab[7]
            got = fit.cv_core(th, None if layout == "loo" else lab)
            check("dense", got, 300, layout, r)
    finally:
        fit.close()


def test_n130_front_padding():
    """n = 130: one tile plus 2, placeholders in front of the observations: leave-one-out and 2 folds of 65"""
    fit, th = fit_for(130, 3)
    try:
        check("dense", fit.cv_core(th), 130, "loo", 3)
        lab = reference(130, "two")[0]
        assert sorted(np.bincount(lab)) == [65, 65]
        check("dense", fit.cv_core(th, lab), 130, "two", 3)
    finally:
        fit.close()


def test_n700_every_regime_in_one_call():
    """folds of 1, 2, 16, 17, 127, 128, 129 observations and the rest (280) in one call: the closed form, every size class of
    the LDS kernel at its boundary, and two folds on the library's factorisation"""
    fit, th = fit_for(700, 3)
    try:
        lab = reference(700, "mixed")[0]
        assert sorted(np.bincount(lab)) == [1, 2, 16, 17, 127, 128, 129, 280]
        check("dense", fit.cv_core(th, lab), 700, "mixed", 3)
    finally:
        fit.close()


def test_n2116_loo_and_two_large_folds():
    """n = 2116: leave-one-out, and 2 folds of 1058 (a nine-tile scratch matrix with a multi-tile border)"""
    fit, th = fit_for(2116, 1)
    try:
        check("dense", fit.cv_core(th), 2116, "loo", 1)
        lab = reference(2116, "two")[0]
        assert sorted(np.bincount(lab)) == [1058, 1058]
        check("dense", fit.cv_core(th, lab), 2116, "two", 1)
    finally:
        fit.close()


@pytest.mark.parametrize("nu", [0.5, 1.5])
def test_fixed_smoothness(nu):
    fit, th = fit_for(300, 1, nu)
    try:
        lab = reference(300, "random10", nu)[0]
        check("nu=%.1f" % nu, fit.cv_core(th, lab), 300, "random10", 1, nu)
    finally:
        fit.close()


def test_repeatability_and_independence():
    """Two calls give identical bits; other names for the folds give identical bits; merging two OTHER folds leaves a fold's
    bits unchanged (small and large folds); singleton folds equal fold = NULL bit for bit (both take the closed form)."""
    n = 700
    fit, th = fit_for(n, 3)
    try:
        lab = reference(n, "mixed")[0]
        first = fit.cv_core(th, lab)
        again = fit.cv_core(th, lab)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        renamed = fit.cv_core(th, (3 * lab + 5) % 11)            # (a bijection on 0 .. 7 into 0 .. 10: empty labels between)
        assert np.unique((3 * np.arange(8) + 5) % 11).size == 8
        assert np.array_equal(first[0], renamed[0]) and np.array_equal(first[1], renamed[1])
        sizes = np.bincount(lab)
        f16, f129 = int(np.nonzero(sizes == 16)[0][0]), int(np.nonzero(sizes == 129)[0][0])
        f17, f127 = int(np.nonzero(sizes == 17)[0][0]), int(np.nonzero(sizes == 127)[0][0])
        merged = np.where(lab == f17, f127, lab)                 # 17 + 127 = 144: two small folds become one large fold
        other = fit.cv_core(th, merged)
        for keep in (f16, f129):
            rows = lab == keep
            assert np.array_equal(first[0][rows], other[0][rows]) and np.array_equal(first[1][rows], other[1][rows])
        assert not np.array_equal(first[1][lab == f17], other[1][lab == f17])
        loo = fit.cv_core(th)
        single = fit.cv_core(th, np.arange(n))
        assert np.array_equal(loo[0], single[0]) and np.array_equal(loo[1], single[1])
        one = lab == int(np.nonzero(sizes == 1)[0][0])
        assert np.array_equal(loo[0][one], first[0][one]) and np.array_equal(loo[1][one], first[1][one])
    finally:
        fit.close()


def test_handle_state_is_untouched():
    """n = 1000: value, gradient, Fisher information and a prepared kriging state give the same bits before and after a
    cross-validation call with folds of every regime; no hand-off time-out on the handle."""
    n = 1000
    fit, th = fit_for(n, 1)
    rng = np.random.default_rng(77)
    lp = rng.uniform(0, 1, size=(40, 2))
    Xp = np.column_stack([np.ones(40), rng.standard_normal(40), rng.standard_normal(40)])
    dirs = np.eye(18)[:3]
    lab = np.concatenate([np.zeros(300, int), np.arange(1, 71).repeat(10)])      # one fold of 300, 70 folds of 10

    def state():
        fit.krige_prepare(th)
        out = [fit.neg2loglik_core(th), fit.neg2loglik_grad_core(th), fit.fisher_core(th, dirs), fit.krige_core(lp, Xp)]
        return [np.asarray(a) for group in out for a in group]

    try:
        fit.krige_prepare(th)
        k0 = fit.krige_core(lp, Xp)
        before = state()
        cv = fit.cv_core(th, lab)
        k1 = fit.krige_core(lp, Xp)                    # the state prepared before the call, applied after it
        cv_loo = fit.cv_core(th)
        after = state()
        eng = fit.engine_state()
    finally:
        fit.close()
    assert all(np.array_equal(a, b) for a, b in zip(k0, k1))
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
    assert eng["retries"] == 0 and eng["last_abort"] == 0, eng
    assert np.all(cv[1] > 0) and np.all(cv_loo[1] > 0) and np.all(cv_loo[1] <= cv[1] * (1 + 1e-9))      # (conditioning on more never adds variance)


def test_failure_paths():
    """A theta whose first minor fails returns k > 0 and writes nothing, and the next call gives the first call's bits; a label
    out of range, a fold of all n, and taper / sharded / no-z handles are refused with -1 and a message naming the entry."""
    from cocons_amd import CoconsTaperFit, _lib, workloads as wl
    from cocons_amd.host import _f, _ip, _p, theta_table
    from test_gpu_grad import _zero_matrix_theta
    n = 300
    fit, th = fit_for(n, 1)
    locs, X, _, z, *_ = problem(n)
    T, mean = theta_table(th), np.ascontiguousarray(th["mean"])
    lab = np.ascontiguousarray(reference(n, "random10")[0], dtype=np.int32)
    resid, var = np.full(n, -7.0), np.full(n, -7.0)

    def refused(h, nfold, fold, word, L=None):
        L = L or fit._L
        assert L.cocons_cv_dense(h, _p(T), _p(mean), nfold, None if fold is None else _ip(fold), _p(resid), _p(var)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_cv_dense:") and word in msg, msg

    try:
        first = fit.cv_core(th, lab)
        bad = _zero_matrix_theta(th)
        rc = fit._L.cocons_cv_dense(fit._h, _p(theta_table(bad)), _p(mean), 10, _ip(lab), _p(resid), _p(var))
        assert rc > 0 and np.all(resid == -7.0) and np.all(var == -7.0)
        again = fit.cv_core(th, lab)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        refused(fit._h, 9, lab, "outside")                                   # label 9 with nfold = 9
        neg = lab.copy()
        neg[5] = -1
        refused(fit._h, 10, neg, "outside")
        refused(fit._h, 3, np.full(n, 2, dtype=np.int32), "holds all")
        noop_b = _lib.BCAST_FN(lambda *a: 0)
        noop_r = _lib.ALLREDUCE_FN(lambda *a: 0)
        assert fit._L.cocons_fit_set_collectives(fit._h, 0, 2, ctypes.cast(noop_b, ctypes.c_void_p),
                                                 ctypes.cast(noop_r, ctypes.c_void_p), None) == 0
        refused(fit._h, 10, lab, "sharded")
    finally:
        fit.close()
    ci, rp = np.arange(1, n + 1, dtype=np.int32), np.arange(1, n + 2, dtype=np.int32)
    tf = CoconsTaperFit(locs, X, z[:, :1], wl.SMOOTH_LIMITS, ci, rp, np.ones(n))
    try:
        refused(tf._h, 10, lab, "taper", tf._L)
    finally:
        tf.close()
    L = _lib.load()
    lf, Xf, sl = _f(locs), _f(X), np.array(wl.SMOOTH_LIMITS, float)
    h = L.cocons_fit_create(n, 3, 0, 0, _p(lf), _p(Xf), None, None, _p(sl), -1)
    assert h
    try:
        refused(h, 0, None, "no z", L)
    finally:
        L.cocons_fit_destroy(h)
    assert np.all(resid == -7.0) and np.all(var == -7.0)


def test_host_and_glue():
    """host.cocoCV_dense with string labels equals cv_core; the glue's _cocons_hip_cv through the R stub equals cv_core bit
    for bit (folds and leave-one-out)."""
    from cocons_amd import host, workloads as wl
    from test_glue_exec import RStub
    n = 300
    fit, th = fit_for(n, 3)
    locs, X, _, z, *_ = problem(n)
    lab = reference(n, "random10")[0]
    try:
        want = fit.cv_core(th, lab)
        want_loo = fit.cv_core(th)
        names = np.array(["fold-%c" % "jihgfedcba"[k] for k in lab])
        out = host.cocoCV_dense(th, locs, X, wl.SMOOTH_LIMITS, z, fold=names, fit=fit)
        own = host.cocoCV_dense(th, locs, X, wl.SMOOTH_LIMITS, z, fold=names)
    finally:
        fit.close()
    for o in (out, own):
        assert np.array_equal(o["resid"], want[0]) and np.array_equal(o["sd.pred"], np.sqrt(want[1]))
        assert np.array_equal(o["mean.pred"], z - want[0])
    crps = host.getCRPS(z, out["mean.pred"], out["sd.pred"][:, None])
    assert crps.shape == (n, 3) and np.all(crps > 0)
    R = RStub()
    h = R.call("_cocons_hip_fit_create", R.real(locs), R.real(X), R.real(z), R.nil, R.real(list(wl.SMOOTH_LIMITS)), R.integer([0]))
    for fold, ref in ((R.integer(lab), want), (R.nil, want_loo)):
        st, got = R.value(R.call("_cocons_hip_cv", h, R.theta(th), R.real(th["mean"]), fold))
        assert int(st[0]) == 0
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    with pytest.raises(RuntimeError, match="cocons_cv_taper"):
        R.call("_cocons_hip_cv_taper", h, R.theta(th), R.real(th["mean"]))
    R.call("_cocons_hip_fit_close", h)
    R.L.stub_gc(0, None)
