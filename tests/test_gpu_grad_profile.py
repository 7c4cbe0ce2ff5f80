"""Analytic gradients of the Profile and REML -2 log-likelihoods on the GPU (cocons_neg2loglik_profile_grad / _reml_grad):
against the numpy statement (tests/grad_profile_reference.py), against the value entries on the same handle, against the GPU's
own Richardson differences, the exact scaling identities, fixed smoothness, odd sizes, isolation from the handle's other work,
failing minors, refusals and the host entries.  Tolerances and sizes are those tests/test_gpu_grad.py holds the dense
gradient to.  Measured on an MI355X: reference 5e-11 of the largest entry or better, Richardson 1.3e-9, identities 2e-12 r n
(n = 2116) and 4e-13 r n (n = 10^4), host gradient 7e-10."""
import ctypes
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_profile_reference as GPR  # noqa: E402
from test_gpu_grad import SHAPES, _general_problem, _zero_matrix_theta  # noqa: E402

pytestmark = pytest.mark.gpu

OBJECTIVES = ("pml", "reml")


def _setup(n, r, seed=3, coincident=False):
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(n, 2))
    if coincident:
        locs[7] = locs[3]
    X = wl.design_from_locs(locs)["std.covs"]
    if coincident:
        X[7] = X[3] + [0.0, 0.5, 0.5]
    th = wl.theta_full(scale0=np.log(0.2))
    z = rng.standard_normal((n, r)) + 0.4 * X[:, [1]] - 0.2
    return locs, X, th, z


def _fit(locs, X, z, q=3, sl=None):
    from cocons_amd import CoconsFit, workloads as wl
    return CoconsFit(locs, X, z, wl.SMOOTH_LIMITS if sl is None else sl, x_betas=np.ascontiguousarray(X[:, :q]) if q else None)


def _inf(a):
    return float(np.max(np.abs(a)))


def _grad(fit, obj, th):
    return fit.neg2loglik_profile_grad_core(th) if obj == "pml" else fit.neg2loglik_reml_grad_core(th, 3)


def _value(fit, obj, th):
    return fit.neg2loglik_profile_core(th) if obj == "pml" else fit.neg2loglik_reml_core(th, 3)


def _reference(obj, th, locs, X, z, q, sl=None):
    from cocons_amd import workloads as wl
    sl = wl.SMOOTH_LIMITS if sl is None else sl
    if obj == "pml":
        return GPR.profile_grad(th, locs, X, z, X[:, :q], sl)
    return GPR.reml_grad(th, locs, X, z, sl)


def _check_reference(obj, n, r, q, coincident=False, sl=None, th_edit=None):
    locs, X, th, z = _setup(n, r, coincident=coincident)
    if th_edit:
        th_edit(th)
    fit = _fit(locs, X, z, q, sl)
    try:
        val, parts, gt = _grad(fit, obj, th)
    finally:
        fit.close()
    f, rgt, beta, quad = _reference(obj, th, locs, X, z, q, sl)
    print(obj, n, r, q, "value", abs(val - f) / abs(f), "gradient", _inf(gt - rgt) / _inf(rgt))
    assert abs(val - f) <= 1e-10 * abs(f)
    assert _inf(gt - rgt) <= 1e-7 * _inf(rgt), (_inf(gt - rgt), _inf(rgt))
    return gt


@pytest.mark.parametrize("n,r", [(300, 1), (300, 3), (2116, 1), (2116, 3)])
@pytest.mark.parametrize("obj,q", [("pml", 2), ("pml", 3), ("reml", 3)])
def test_against_reference(obj, q, n, r):
    _check_reference(obj, n, r, q, coincident=(n == 300))


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_value_parts_and_repeats(obj):
    n, r = 300, 2
    locs, X, th, z = _setup(n, r)
    fit = _fit(locs, X, z, 2)
    try:
        val, parts, gt = _grad(fit, obj, th)
        val2, parts2, gt2 = _grad(fit, obj, th)
        vval, vparts = _value(fit, obj, th)
    finally:
        fit.close()
    assert parts.shape == vparts.shape
    assert abs(val - vval) <= 1e-12 * abs(vval)
    assert np.max(np.abs(parts - vparts) / np.abs(vparts)) <= 1e-12, (parts, vparts)
    assert val == val2 and np.array_equal(parts, parts2) and np.array_equal(gt, gt2)


@pytest.mark.parametrize("n", [2116, 4096])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_against_gpu_richardson(obj, n):
    from cocons_amd import host
    locs, X, th, z = _setup(n, 1, seed=5)
    fit = _fit(locs, X, z)
    try:
        val, parts, gt = _grad(fit, obj, th)
        h = 1e-4
        v = np.zeros((18, 4))
        for t in range(6):
            for k in range(3):
                for j, s in enumerate((h, -h, h / 2, -h / 2)):
                    tl = OrderedDict((kk, np.array(vv, float)) for kk, vv in th.items())
                    tl[host.COV_ASPECTS[t]][k] += s
                    v[3 * t + k, j] = _value(fit, obj, tl)[0]
    finally:
        fit.close()
    num = (4 * (v[:, 2] - v[:, 3]) / h - (v[:, 0] - v[:, 1]) / (2 * h)) / 3
    print(obj, n, "error", _inf(gt.ravel() - num) / _inf(num))
    assert _inf(gt.ravel() - num) <= 1e-6 * _inf(num), (gt.ravel(), num)


@pytest.mark.parametrize("n,tol", [(2116, 1e-9), (10000, 1e-8)])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_scaling_identity(obj, n, tol):
    """Sigma(sd0 + d, ng0 + d) = e^d Sigma: d f / d sd0 + d f / d ng0 = r n_eff - sum_k quad_k, n_eff = n (Profile), n - p (REML)."""
    r = 1
    locs, X, th, z = _setup(n, r, seed=9)
    fit = _fit(locs, X, z)
    try:
        val, parts, gt = _grad(fit, obj, th)
    finally:
        fit.close()
    lhs = gt[0, 0] + gt[5, 0]
    rhs = r * (n if obj == "pml" else n - 3) - np.sum(parts[2:2 + r])
    print(obj, n, "identity", abs(lhs - rhs) / (r * n))
    assert abs(lhs - rhs) <= tol * r * n, (lhs, rhs)


@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, 1.0])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_fixed_smoothness(obj, nu):
    def edit(th):
        th["smooth"] = np.zeros(3)
        if nu == 1.0:               # hi == lo on the general branch: a varying smooth vector with zero span
            th["smooth"] = np.array([0.0, 0.5, -0.5])

    gt = _check_reference(obj, 300, 1, 3, sl=(nu, nu), th_edit=edit)
    assert np.all(gt[4] == 0.0)


@pytest.mark.parametrize("n", [1000, 2117])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_odd_sizes(obj, n):
    _check_reference(obj, n, 1, 3)


@pytest.mark.parametrize("n,p,r", SHAPES)
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_shapes_against_reference(obj, n, p, r):
    """The shapes of tests/test_gpu_grad.py::test_shapes_against_reference (p from 1 to 32, n from 1 across the tile edges,
    r = 1 and 3); Profile with q = max(1, p // 2) columns of x_betas.  Tolerances of test_against_reference; a failing first
    minor returns its index and leaves every output untouched; the next call gives the first call's bits."""
    from cocons_amd import CoconsFit, workloads as wl
    from cocons_amd.host import _p, theta_table
    locs, X, th, z = _general_problem(n, p, r, 7000 + 40 * n + p)
    z = z + 0.4 * X[:, [p - 1]] - 0.2
    q = max(1, p // 2) if obj == "pml" else p
    xb = np.ascontiguousarray(X[:, :q])

    def grad(t):
        return fit.neg2loglik_profile_grad_core(t) if obj == "pml" else fit.neg2loglik_reml_grad_core(t, p)

    fit = CoconsFit(locs, X, z, wl.SMOOTH_LIMITS, x_betas=xb)
    try:
        val, parts, gt = grad(th)
        T = theta_table(_zero_matrix_theta(th))
        v7 = ctypes.c_double(7.0)
        p7, g7 = np.full(2 + r + q, 7.0), np.full(6 * p, 7.0)
        if obj == "pml":
            rc = fit._L.cocons_neg2loglik_profile_grad(fit._h, _p(T), ctypes.byref(v7), _p(p7), _p(g7))
        else:
            rc = fit._L.cocons_neg2loglik_reml_grad(fit._h, _p(T), p, ctypes.byref(v7), _p(p7), _p(g7))
        assert rc == 1
        assert v7.value == 7.0 and np.all(p7 == 7.0) and np.all(g7 == 7.0)
        again = grad(th)
    finally:
        fit.close()
    assert again[0] == val and np.array_equal(again[1], parts) and np.array_equal(again[2], gt)
    assert gt.shape == (6, p) and parts.shape == (2 + r + q,)
    if obj == "pml":
        f, rgt, beta, quad = GPR.profile_grad(th, locs, X, z, xb, wl.SMOOTH_LIMITS)
    else:
        f, rgt, beta, quad = GPR.reml_grad(th, locs, X, z, wl.SMOOTH_LIMITS)
    if obj == "reml" and n == p:
        # no residual degree of freedom: log det Sigma + log det W = 2 log |X| and the quadratic forms vanish, so the
        # objective is constant in theta (r log x^2 at n = p = 1) and its gradient zero.  Relative tolerances have nothing
        # to refer to: the same fractions of what cancels instead -- r |log det Sigma| + r |log det W| in the value, r Sigma^-1
        # dSigma = O(r) per table entry in the gradient
        print(obj, n, p, r, "constant objective: value", val, f, "gradient", _inf(gt))
        assert _inf(rgt) <= 1e-12 * r
        assert abs(val - f) <= 1e-10 * 2 * r * (abs(parts[0]) + abs(parts[1]) + 1.0)
        assert _inf(gt) <= 1e-7 * r, gt
        return
    print(obj, n, p, r, "value", abs(val - f) / abs(f), "gradient", _inf(gt - rgt) / _inf(rgt))
    assert abs(val - f) <= 1e-10 * abs(f)
    assert _inf(gt - rgt) <= 1e-7 * _inf(rgt), (_inf(gt - rgt), _inf(rgt))


def _fit_memory(fit):
    out = (ctypes.c_longlong * 4)()
    assert fit._L.cocons_debug_fit_memory(fit._h, out) == 0
    return list(out)


def test_isolation_on_one_handle():
    from cocons_amd import workloads as wl
    n = 2116
    locs, X, th, z = _setup(n, 1, seed=4)
    npad = (n + 127) // 128 * 128
    fit = _fit(locs, X, z)
    try:
        fit.krige_prepare(th)
        lp = np.random.default_rng(1).uniform(0, 1, size=(200, 2))
        Xp = wl.design_from_locs(lp)["std.covs"]
        s0, q0 = fit.krige_core(lp, Xp)
        v0, p0 = fit.neg2loglik_core(th)
        m0 = _fit_memory(fit)
        d1 = fit.neg2loglik_grad_core(th)
        m1 = _fit_memory(fit)
        gp = fit.neg2loglik_profile_grad_core(th)
        d2 = fit.neg2loglik_grad_core(th)
        gr = fit.neg2loglik_reml_grad_core(th, 3)
        d3 = fit.neg2loglik_grad_core(th)
        v1, p1 = fit.neg2loglik_core(th)
        m2 = _fit_memory(fit)
        s1, q1 = fit.krige_core(lp, Xp)
    finally:
        fit.close()
    for d in (d2, d3):
        assert d[0] == d1[0] and all(np.array_equal(a, b) for a, b in zip(d[1:], d1[1:]))
    assert v1 == v0 and np.array_equal(p1, p0)
    assert 0 < m1[0] - m0[0] <= npad * npad * 8
    assert m2[0] == m1[0]                                   # dA grown once, by the dense gradient's layout
    assert m2[3] == m0[3] and m2[1] == m0[1]                # the objective's leading dimension and dP unchanged
    assert np.array_equal(s0, s1) and np.array_equal(q0, q1)
    assert np.all(np.isfinite(gp[2])) and np.all(np.isfinite(gr[2]))


def _bad_theta(th):
    bad = OrderedDict((k, np.array(v, float)) for k, v in th.items())
    bad["nugget"] = np.array([-np.inf, 0.0, 0.0])
    bad["scale"][0] = np.log(50.0)             # a near-constant covariance without nugget: not positive definite
    return bad


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_failing_minor_then_success(obj):
    from cocons_amd import CholeskyError
    from cocons_amd.host import _p, theta_table
    n = 1000
    locs, X, th, z = _setup(n, 1)
    fit = _fit(locs, X, z)
    try:
        T = theta_table(_bad_theta(th))
        val = ctypes.c_double(7.0)
        parts, gt = np.full(6, 7.0), np.full(18, 7.0)
        if obj == "pml":
            rc = fit._L.cocons_neg2loglik_profile_grad(fit._h, _p(T), ctypes.byref(val), _p(parts), _p(gt))
        else:
            rc = fit._L.cocons_neg2loglik_reml_grad(fit._h, _p(T), 3, ctypes.byref(val), _p(parts), _p(gt))
        assert rc > 0
        assert val.value == 7.0 and np.all(parts == 7.0) and np.all(gt == 7.0)
        with pytest.raises(CholeskyError):
            _grad(fit, obj, _bad_theta(th))
        v1 = _grad(fit, obj, th)
        v0, _ = _value(fit, obj, th)
        assert abs(v1[0] - v0) <= 1e-12 * abs(v0)
    finally:
        fit.close()


def test_refusals():
    from cocons_amd import CoconsTaperFit, workloads as wl, _lib
    from cocons_amd.host import _p, theta_table
    n = 200
    locs, X, th, z = _setup(n, 1)
    ci = np.arange(1, n + 1, dtype=np.int32)
    rp = np.arange(1, n + 2, dtype=np.int32)
    T = theta_table(th)
    val, parts, gt = ctypes.c_double(0), np.zeros(6), np.zeros(18)

    def both(h, L):
        return ((L.cocons_neg2loglik_profile_grad(h, _p(T), ctypes.byref(val), _p(parts), _p(gt)), "cocons_neg2loglik_profile_grad"),
                (L.cocons_neg2loglik_reml_grad(h, _p(T), 3, ctypes.byref(val), _p(parts), _p(gt)), "cocons_neg2loglik_reml_grad"))

    tf = CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, np.ones(n))
    try:
        L = tf._L
        rc = L.cocons_neg2loglik_profile_grad(tf._h, _p(T), ctypes.byref(val), _p(parts), _p(gt))
        assert rc == -1 and _lib.last_error().startswith("cocons_neg2loglik_profile_grad")
        rc = L.cocons_neg2loglik_reml_grad(tf._h, _p(T), 3, ctypes.byref(val), _p(parts), _p(gt))
        assert rc == -1 and _lib.last_error().startswith("cocons_neg2loglik_reml_grad")
    finally:
        tf.close()
    fit = _fit(locs, X, z, q=0)                  # no x_betas: Profile refused, REML runs
    try:
        L = fit._L
        rc = L.cocons_neg2loglik_profile_grad(fit._h, _p(T), ctypes.byref(val), _p(parts), _p(gt))
        assert rc == -1 and _lib.last_error().startswith("cocons_neg2loglik_profile_grad") and "x_betas" in _lib.last_error()
        assert L.cocons_neg2loglik_reml_grad(fit._h, _p(T), 3, ctypes.byref(val), _p(parts), _p(gt)) == 0
    finally:
        fit.close()
    fit = _fit(locs, X, z)
    try:
        L = fit._L
        noop_b = _lib.BCAST_FN(lambda *a: 0)
        noop_r = _lib.ALLREDUCE_FN(lambda *a: 0)
        assert L.cocons_fit_set_collectives(fit._h, 0, 2, ctypes.cast(noop_b, ctypes.c_void_p),
                                            ctypes.cast(noop_r, ctypes.c_void_p), None) == 0
        for rc, name in both(fit._h, L):
            assert rc == -1, name
        assert "sharded" in _lib.last_error()
    finally:
        fit.close()


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_host_entries(obj):
    """host.GetNeg2loglikelihoodProfile_grad / ...REML_grad: value against the value function (penalty included), gradient over
    the optimiser's vector (par_pos["mean"] all False) against Richardson differences of it, and the (1e6, zeros) /
    RuntimeError paths of a failing Cholesky."""
    from cocons_amd import host, workloads as wl
    n = 300
    locs, X, th, z = _setup(n, 1)
    z = z[:, 0]
    pp = wl.par_pos_full()
    pp["mean"] = [False] * 3
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.7, 0.3, 0.2)
    sl = wl.SMOOTH_LIMITS

    def run(fun_p, fun_r, x, fit, **kw):
        if obj == "pml":
            return fun_p(x, pp, locs, X, sl, z, n, X, lam, fit=fit, **kw)
        return fun_r(x, pp, locs, X, X, sl, z, n, lam, fit=fit, **kw)

    fit = _fit(locs, X, z)
    try:
        def val(x):
            return run(host.GetNeg2loglikelihoodProfile, host.GetNeg2loglikelihoodREML, x, fit, safe=False)

        v, g = run(host.GetNeg2loglikelihoodProfile_grad, host.GetNeg2loglikelihoodREML_grad, x0, fit, safe=False)
        assert abs(v - val(x0)) <= 1e-12 * abs(v)
        h = 1e-4
        num = np.zeros_like(x0)
        for i in range(x0.size):
            def d(step):
                xp, xm = x0.copy(), x0.copy()
                xp[i] += step
                xm[i] -= step
                return (val(xp) - val(xm)) / (2 * step)
            num[i] = (4 * d(h / 2) - d(h)) / 3
        assert g.shape == x0.shape
        print(obj, "host gradient error", _inf(g - num) / _inf(num))
        assert _inf(g - num) <= 1e-6 * _inf(num), (g, num)
    finally:
        fit.close()
    n = 1000
    locs, X, th, z = _setup(n, 1)
    xb = wl.theta_vector_from_lists(_bad_theta(th), pp)
    fit = _fit(locs, X, z)
    try:
        vb, gb = run(host.GetNeg2loglikelihoodProfile_grad, host.GetNeg2loglikelihoodREML_grad, xb, fit)
        assert vb == 1e6 and gb.shape == xb.shape and np.all(gb == 0)
        with pytest.raises(RuntimeError, match="Cholesky error"):
            run(host.GetNeg2loglikelihoodProfile_grad, host.GetNeg2loglikelihoodREML_grad, xb, fit, safe=False)
    finally:
        fit.close()
