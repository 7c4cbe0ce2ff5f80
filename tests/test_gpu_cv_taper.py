"""cocons_cv_taper on the GPU -- leave-one-out predictions of the tapered model S = T o C(theta) from the selected inverse --
against the numpy statement of tests/cv_reference.py on the dense S of tests/grad_taper_reference.py: brute force (one
Cholesky per observation) up to n = 700, the route through the dense inverse at n = 1500 (tests/test_cv_reference.py pins
the two to each other).  Bound: 1e-8 in gap_e = max |resid - resid_ref| / sd_ref and gap_v = max |var - var_ref| / var_ref."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
import grad_taper_reference as GT  # noqa: E402
from test_gpu_grad_taper import _delta, _setup, _taper_fit  # noqa: E402
from test_gpu_parity import _taper_pattern  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 1e-8


def _reference(th, locs, X, z, ref_taper, brute):
    from cocons_amd import workloads as wl
    from cocons_amd.host import theta_table
    S, _ = GT.taper_matrix(theta_table(th), locs, X, wl.SMOOTH_LIMITS, ref_taper)
    S = np.tril(S) + np.tril(S, -1).T                   # (the library reads the lower triangle)
    R = z - (X @ th["mean"])[:, None]
    return (CV.cv_brute if brute else CV.cv_kroute)(S, R, np.arange(X.shape[0]))


def _check(tag, got, ref):
    ge, gv = CV.gaps(got[0], got[1], ref[0], ref[1])
    print("%s: gap_e %.3e gap_v %.3e (var %.3g .. %.3g)" % (tag, ge, gv, ref[1].min(), ref[1].max()))
    assert ge <= BOUND and gv <= BOUND, (ge, gv)


@pytest.mark.parametrize("n,r", [(150, 1), (700, 2), (1500, 1)])
def test_leave_one_out_vs_reference(n, r):
    """two tiles, several tiles, the packed band buffer; two calls give identical bits; value and taper gradient before and
    after are bit-identical"""
    locs, X, th, z, _ = _setup(n, r)
    ref_taper = _taper_pattern(locs, _delta(n))
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        v0, g0 = fit.neg2loglik_core(th), fit.neg2loglik_grad_core(th)
        got = fit.cv_core(th)
        again = fit.cv_core(th)
        v1, g1 = fit.neg2loglik_core(th), fit.neg2loglik_grad_core(th)
    finally:
        fit.close()
    assert got[0].shape == (n, r) and got[1].shape == (n,)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    assert v1[0] == v0[0] and np.array_equal(v1[1], v0[1])
    assert g1[0] == g0[0] and all(np.array_equal(a, b) for a, b in zip(g1[1:], g0[1:]))
    _check("taper n=%d r=%d" % (n, r), got, _reference(th, locs, X, z, ref_taper, brute=n <= 700))


def test_duplicated_location(monkeypatch):
    """the duplicated-location case of test_gpu_grad_taper.py (caller's order, so that the pair's entry is the reference's)"""
    monkeypatch.setenv("COCONS_TAPER_RCM", "0")
    n, r = 700, 1
    locs, X, th, z, _ = _setup(n, r, seed=31)
    locs[400] = locs[5]
    X[400] = X[5]
    X[5] = X[5] + [0.0, 0.5, 0.0]
    ref_taper = _taper_pattern(locs, 0.25)
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        got = fit.cv_core(th)
    finally:
        fit.close()
    ref = _reference(th, locs, X, z, ref_taper, brute=True)
    _check("taper duplicate", got, ref)
    assert ref[1][[5, 400]].max() < np.median(ref[1])      # (each of the two is predicted from the other)


def test_dense_handle_refused_and_host_layer():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    from cocons_amd.host import _p, theta_table
    n, r = 150, 2
    locs, X, th, z, _ = _setup(n, r)
    ref_taper = _taper_pattern(locs, 0.25)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    resid, var = np.full(n * r, -7.0), np.full(n, -7.0)
    try:
        rc = dense._L.cocons_cv_taper(dense._h, _p(theta_table(th)), _p(np.ascontiguousarray(th["mean"])), _p(resid), _p(var))
        assert rc == -1 and _lib.last_error().startswith("cocons_cv_taper:") and "not a taper fit" in _lib.last_error()
    finally:
        dense.close()
    assert np.all(resid == -7.0) and np.all(var == -7.0)
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        want = fit.cv_core(th)
        out = host.cocoCV_sparse(th, locs, X, wl.SMOOTH_LIMITS, z, ref_taper, fit=fit)
    finally:
        fit.close()
    own = host.cocoCV_sparse(th, locs, X, wl.SMOOTH_LIMITS, z, ref_taper)
    for o in (out, own):
        assert np.array_equal(o["resid"], want[0]) and np.array_equal(o["sd.pred"], np.sqrt(want[1]))
        assert np.array_equal(o["mean.pred"], z - want[0])
