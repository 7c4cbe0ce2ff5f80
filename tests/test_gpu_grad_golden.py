"""The analytic gradients on the GPU against exact-arithmetic golden vectors (tests/golden/make_golden_grad.py: 70-digit
central differences of the whole objective, nothing of grad.hip's pair-partial algebra restated), and matern_pair /
matern_dnu against the exact Matern partials on a (nu, u) grid.

Bounds.  Per family (a row of the 6 x p table; the mean vector is its own family) the device's error, as a fraction of the
family's largest golden component, must not exceed

    max(10 x ref_err[family], 1e-13),  and never the 1e-7 of tests/test_gpu_grad.py,

where ref_err is the error of the float64 numpy statement of the same gradient against the same golden (measured on the CPU,
stored in the fixture, asserted <= 1e-11 / 1e-8 (smooth) by tests/test_grad_golden.py).  The factor 10 allows for a different,
equally valid, fixed summation order of the same fp64 work.  Value and parts: 1e-12 relative.  A golden row that is exactly
zero (nugget off; fixed smoothness; the taper model's aniso and tilt rows) must be exactly zero on the device.

Pointwise: M and dM/du within 2e-13 relative wherever |golden| > 1e-290 (the bound test_device_matern_large_orders_vs_mpmath
holds the same continued fraction to); |dM/dnu - golden| <= dnu_trunc + 1.5 x 2e-13 |M| / (1e-3 nu): the exact truncation
of the four-point stencil plus its weights (sum 18/12 over h) times the rounding allowed to each M.
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grad_taper_reference as GT  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = ("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
CASES = ("base", "tiles", "wide", "low", "nonugget", "far", "nu1p5", "nu1")


def load(fname):
    with open(os.path.join(HERE, "golden", fname)) as f:
        return json.load(f)


def theta_of(fx):
    th = OrderedDict()
    for k in ("mean",) + ROWS:
        th[k] = np.array([(-np.inf if v == "-inf" else v) for v in fx["theta"][k]], dtype=float)
    return th


def bound(ref_err):
    return min(max(10.0 * ref_err, 1e-13), 1e-7)


def check_values(label, val, parts, gold_val, gold_parts, nbeta=0):
    gold_parts = np.asarray(gold_parts, dtype=float)
    m = gold_parts.size - nbeta
    rel = np.abs(parts[:m] - gold_parts[:m]) / np.abs(gold_parts[:m])
    print("%s value %.2e parts %.2e" % (label, abs(val - gold_val) / abs(gold_val), rel.max()))
    assert abs(val - gold_val) <= 1e-12 * abs(gold_val), label
    assert rel.max() <= 1e-12, (label, rel)
    if nbeta:                   # the GLS coefficients, one solve: relative to the vector's largest component
        b, gb = parts[m:], gold_parts[m:]
        assert np.max(np.abs(b - gb)) <= 1e-12 * np.max(np.abs(gb)), (label, b, gb)


def check_families(label, got_table, gold_table, ref_err, got_mean=None, gold_mean=None):
    rows = list(zip(ROWS, np.asarray(got_table), np.asarray(gold_table, dtype=float)))
    if gold_mean is not None:
        rows.append(("mean", np.asarray(got_mean), np.asarray(gold_mean, dtype=float)))
    bad = []
    for fam, g, w in rows:
        scale = float(np.max(np.abs(w)))
        if scale == 0.0:
            print("%s %-8s golden row exactly zero, device %s" % (label, fam, g))
            assert np.all(g == 0.0), (label, fam, g)
            continue
        err = float(np.max(np.abs(g - w))) / scale
        b = bound(ref_err[fam])
        print("%s %-8s device %.3e ref_err %.3e bound %.3e%s" % (label, fam, err, ref_err[fam], b, "  <-- EXCEEDS" if err > b else ""))
        if not err <= b:
            bad.append((fam, err, b))
    assert not bad, (label, bad)


@pytest.mark.parametrize("case", CASES)
def test_dense_profile_reml_vs_golden(case):
    """grad_dense_<case>.json: the dense, Profile (x_betas = two columns of X) and REML gradients of one handle.  base: n = 70,
    r = 2, a coincident pair, a nugget covariate effect; tiles: n = 140 (two factorisation tiles, three pair tiles); wide:
    limits (0.1, 6), nu_ij from below 1/2 to above 3.5; low: limits (0.05, 0.5), every pair on matern_pair's n == 0 branch;
    nonugget: nugget intercept -Inf; far: 86 % of the pairs beyond u = 706 (the stand-in value, zero partials); nu1p5: the
    closed form; nu1: fixed smoothness 1 on the general branch -- a varying smooth vector with zero span, as
    test_fixed_smoothness (a ZERO smooth vector with hi == lo off the half-integers is the reference's quirk u = 0, a
    singular matrix).  Measured on an MI355X: at most 0.49 of a family's bound (tests/golden/GRAD_GOLDEN_REPORT.md)."""
    from cocons_amd import CoconsFit
    fx = load("grad_dense_%s.json" % case)
    th = theta_of(fx)
    r, p = fx["r"], fx["p"]
    xb = np.ascontiguousarray(np.array(fx["x_betas"]))
    fit = CoconsFit(np.array(fx["locs"]), np.array(fx["X"]), np.array(fx["z"]), tuple(fx["smooth_limits"]), x_betas=xb)
    try:
        dense = fit.neg2loglik_grad_core(th)
        dense2 = fit.neg2loglik_grad_core(th)
        prof = fit.neg2loglik_profile_grad_core(th)
        reml = fit.neg2loglik_reml_grad_core(th, fx["reml"]["rank"])
    finally:
        fit.close()
    assert dense[0] == dense2[0] and all(np.array_equal(a, b) for a, b in zip(dense[1:], dense2[1:]))
    failures = []
    for label, res, gold, nbeta in (("dense", dense, fx["dense"], 0), ("profile", prof, fx["profile"], xb.shape[1]),
                                    ("reml", reml, fx["reml"], p)):
        check_values("%s %s" % (case, label), res[0], res[1], gold["value"], gold["parts"], nbeta)
        try:
            check_families("%s %s" % (case, label), res[2], gold["grad_table"], fx["ref_err"][label],
                           res[3] if label == "dense" else None, gold.get("grad_mean"))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


def test_taper_vs_golden(monkeypatch):
    """grad_taper_n150.json: two envelope tiles, r = 2, one duplicated location whose earlier site has the larger variance, in
    the caller's order (COCONS_TAPER_RCM=0, as test_duplicated_location: the pair's entry is the diagonal value of its row
    site on the lower triangle).  grad_theta against the golden's two shares summed, grad_quad against the quadratic-form
    share, grad_mean; the aniso and tilt rows exactly zero."""
    from cocons_amd import CoconsTaperFit
    monkeypatch.setenv("COCONS_TAPER_RCM", "0")
    fx = load("grad_taper_n150.json")
    th = theta_of(fx)
    locs = np.array(fx["locs"])
    ci, rp, ent = GT.wendland1_pattern(locs, fx["delta"])
    assert ci.size == fx["nnz"]
    fit = CoconsTaperFit(locs, np.array(fx["X"]), np.array(fx["z"]), tuple(fx["smooth_limits"]), ci, rp, ent)
    try:
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(th)
        again = fit.neg2loglik_grad_core(th)
    finally:
        fit.close()
    assert again[0] == v and all(np.array_equal(a, b) for a, b in zip(again[1:], (parts, gt, gq, gm)))
    check_values("taper", v, parts, fx["value"], fx["parts"])
    gl, gqd = np.array(fx["grad_logdet"]), np.array(fx["grad_quad"])
    failures = []
    for label, got, want, key, mean in (("taper total", gt, gl + gqd, "total", True), ("taper quad", gq, gqd, "quad", False)):
        try:
            check_families(label, got, want, fx["ref_err"][key], gm if mean else None, fx["grad_mean"] if mean else None)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


def _grid():
    g = load("matern_partials_grid.json")
    nu = np.ascontiguousarray(np.repeat(np.array(g["nu"]), len(g["u"])))
    u = np.ascontiguousarray(np.tile(np.array(g["u"]), len(g["nu"])))
    return nu, u, {k: np.array(g[k]) for k in ("M", "dM_du", "dM_dnu", "dnu_trunc")}


def _device_partials(nu, u):
    from cocons_amd import _lib
    D = _lib.load()
    out = np.zeros(3 * nu.size)
    dp = _lib.c_dp
    assert D.cocons_debug_matern_grad(nu.size, nu.ctypes.data_as(dp), u.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    return out.reshape(3, -1)


def test_matern_value_and_du_on_the_grid():
    """M and dM/du = -2^(1-nu)/Gamma(nu) u^nu K_{nu-1}(u): 2e-13 relative wherever |golden| > 1e-290, nu from 0.01 to 15, u from
    1e-10 to 705.99 -- the n == 0 branch (nu < 1/2) at small u included, where K_{nu-1} used to come from a cancelling
    difference (3e-6 at nu = 0.499999, u = 1e-10)."""
    nu, u, g = _grid()
    M, Mu, _ = _device_partials(nu, u)
    bad = []
    for name, got, want in (("M", M, g["M"]), ("dM/du", Mu, g["dM_du"])):
        ok = np.abs(want) > 1e-290
        rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
        k = int(np.argmax(rel))
        print("%-6s largest relative error %.3e at nu = %g, u = %g; %d of %d points above 2e-13"
              % (name, rel[k], nu[ok][k], u[ok][k], int(np.sum(rel > 2e-13)), rel.size))
        for i in np.nonzero(rel > 2e-13)[0]:
            bad.append((name, nu[ok][i], u[ok][i], rel[i]))
        assert np.all(np.isfinite(got))
    assert not bad, bad


def test_matern_dnu_on_the_grid():
    """|dM/dnu - golden| <= dnu_trunc + 1.5 x 2e-13 |M| / (1e-3 nu) wherever |M| > 1e-290 (below, the stencil's four values
    are subnormal or zero and a bound proportional to |M| has no meaning in doubles)."""
    nu, u, g = _grid()
    _, _, Mn = _device_partials(nu, u)
    ok = np.abs(g["M"]) > 1e-290
    allowed = g["dnu_trunc"] + 1.5 * 2e-13 * np.abs(g["M"]) / (1e-3 * nu)
    ratio = np.abs(Mn - g["dM_dnu"])[ok] / allowed[ok]
    k = int(np.argmax(ratio))
    print("dM/dnu largest error / bound %.3f at nu = %g, u = %g; rounding part alone (error - truncation) / (3e-13 |M| / h): %.3f"
          % (ratio[k], nu[ok][k], u[ok][k],
             np.max((np.abs(Mn - g["dM_dnu"]) - g["dnu_trunc"])[ok] / (allowed - g["dnu_trunc"])[ok])))
    assert np.all(np.isfinite(Mn))
    bad = [(nu[ok][i], u[ok][i], ratio[i]) for i in np.nonzero(ratio > 1.0)[0]]
    assert not bad, bad


def test_matern_partials_beyond_706():
    """u >= 706: M is the reference's stand-in (what cocons_debug_matern returns, bit for bit) and both partials are 0."""
    from cocons_amd import _lib
    nu = np.ascontiguousarray(np.repeat([0.05, 0.45, 0.5, 1.0, 2.5, 5.7, 12.0], 4))
    u = np.ascontiguousarray(np.tile([706.0, 706.0000001, 720.5, 1500.0], 7))
    M, Mu, Mn = _device_partials(nu, u)
    want = np.empty_like(u)
    D = _lib.load()
    assert D.cocons_debug_matern(u.size, nu.ctypes.data_as(_lib.c_dp), u.ctypes.data_as(_lib.c_dp),
                                 want.ctypes.data_as(_lib.c_dp)) == 0
    assert np.array_equal(M, want) and np.all(Mu == 0.0) and np.all(Mn == 0.0)
