"""Expected (Fisher) information of the dense model on the GPU (cocons_fisher_dense): against the numpy / scipy statement
(tests/fisher_reference.py) in the metric max_ab |I_ab - R_ab| / sqrt(R_aa R_bb), the exact scaling identity, symmetry and
positive semi-definiteness, linearity in the directions, fixed smoothness, bit-identical repeats, the handle's other entries
before and after, failing minors, refusals and the host entry getFisher_dense."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-7          # the project's tolerance for the same pair partials (test_gpu_grad.py)


def _setup(n, r, seed=3, coincident=False):
    """the problem of test_gpu_grad._setup"""
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(n, 2))
    if coincident:
        locs[7] = locs[3]
    X = wl.design_from_locs(locs)["std.covs"]
    if coincident:
        X[7] = X[3] + [0.0, 0.5, 0.5]
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = np.array([0.3, -0.15, 0.2])
    z = rng.standard_normal((n, r))
    return locs, X, th, z


def _fit(locs, X, z, sl=None):
    from cocons_amd import CoconsFit, workloads as wl
    return CoconsFit(locs, X, z, wl.SMOOTH_LIMITS if sl is None else sl)


UNITS = np.eye(18).reshape(18, 6, 3)


def _mixes():
    """v_s and six seeded random mixes over all families"""
    rng = np.random.default_rng(41)
    return np.concatenate([FR.scaling_direction(3)[None], rng.standard_normal((6, 6, 3))])


@functools.lru_cache(maxsize=None)
def _reference(n, kind, sl=None, smooth=None):
    """(I at r = 1, X' Sigma^-1 X) of the n-site problem for the 18 unit directions (kind 'units') or the 7 mixes ('mixes'),
    computed once and left unchanged"""
    from cocons_amd import host, workloads as wl
    locs, X, th, _ = _setup(n, 1, coincident=(n == 300))
    if smooth is not None:
        th["smooth"] = np.array(smooth)
    limits = wl.SMOOTH_LIMITS if sl is None else sl
    S, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, limits, UNITS if kind == "units" else _mixes())
    I = FR.info_solve(S, Sa, 1)
    Im = X.T @ np.linalg.solve(S, X)
    I.setflags(write=False)
    Im.setflags(write=False)
    return I, Im


def _check_mean(info_mean, r, locs, X, th, oracle, sl=None):
    from cocons_amd import workloads as wl
    S = oracle.cov_rns(th, locs, X, wl.SMOOTH_LIMITS if sl is None else sl)
    want = r * X.T @ np.linalg.solve(S, X)
    gap = np.max(np.abs(info_mean - want)) / np.max(np.abs(want))
    print("info_mean against the oracle: %.2e" % gap)
    assert gap <= 1e-10


@pytest.mark.parametrize("n,r", [(300, 1), (300, 3), (130, 1)])
def test_unit_directions_against_reference(oracle, n, r):
    locs, X, th, z = _setup(n, r, coincident=(n == 300))
    fit = _fit(locs, X, z)
    try:
        info, info_mean = fit.fisher_core(th, UNITS)
    finally:
        fit.close()
    R, _ = _reference(n, "units")
    gap = FR.metric(info, r * R)
    print("n=%d r=%d gap %.2e" % (n, r, gap))
    assert gap <= TOL
    assert np.array_equal(info, info.T)
    _check_mean(info_mean, r, locs, X, th, oracle)


def test_mixed_directions_against_reference_n2116(oracle):
    """17 tiles of 128: crosses the 256-column blocks of the factorisation, the column panels of the products and the
    plain / engine schedule boundary"""
    n = 2116
    locs, X, th, z = _setup(n, 1)
    fit = _fit(locs, X, z)
    try:
        info, info_mean = fit.fisher_core(th, _mixes())
    finally:
        fit.close()
    R, _ = _reference(n, "mixes")
    gap = FR.metric(info, R)
    print("n=%d gap %.2e; I(v_s, v_s) - n / 2 = %.2e" % (n, gap, info[0, 0] - n / 2))
    assert gap <= TOL
    assert abs(info[0, 0] - n / 2) <= 1e-9 * n
    _check_mean(info_mean, 1, locs, X, th, oracle)


@pytest.mark.parametrize("n,r,tol", [(2116, 3, 1e-9), (4096, 1, 1e-8)])
def test_identities(n, r, tol):
    """no reference needed: I(v_s, v_s) = r n / 2 (Sigma_v = Sigma), symmetry to the bit, positive semi-definiteness"""
    locs, X, th, z = _setup(n, r, seed=9)
    fit = _fit(locs, X, z)
    try:
        info, info_mean = fit.fisher_core(th, _mixes())
    finally:
        fit.close()
    print("n=%d r=%d I(v_s, v_s) - r n / 2 = %.2e" % (n, r, info[0, 0] - r * n / 2))
    assert abs(info[0, 0] - r * n / 2) <= tol * n
    assert np.array_equal(info, info.T)
    d = np.sqrt(np.diag(info))
    assert np.all(d > 0)
    lam = np.linalg.eigvalsh(info / np.outer(d, d))[0]
    print("smallest eigenvalue of the normalised matrix %.3e" % lam)
    assert lam >= -1e-10
    assert np.array_equal(info_mean, info_mean.T) and np.linalg.eigvalsh(info_mean)[0] > 0


def test_direction_linearity():
    """the row of 0.5 (e_a + e_b) is 0.5 (row a + row b): pairs across scale k = 0 / k >= 1 and across families"""
    n = 300
    locs, X, th, z = _setup(n, 1, coincident=True)
    flat = np.eye(18)
    pairs = [(3, 4), (3, 5), (4, 5), (0, 3), (0, 4), (15, 1), (12, 9)]       # (t * 3 + k)
    V = np.concatenate([flat, np.stack([0.5 * (flat[a] + flat[b]) for a, b in pairs])])
    fit = _fit(locs, X, z)
    try:
        info, _ = fit.fisher_core(th, V)
    finally:
        fit.close()
    want = V @ info[:18, :18] @ V.T
    gap = FR.metric(info, want)
    print("linearity gap %.2e" % gap)
    assert gap <= 1e-12


@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, 1.0])
def test_fixed_smoothness(nu):
    n = 300
    locs, X, th, z = _setup(n, 1, coincident=True)
    smooth = (0.0, 0.0, 0.0)
    if nu == 1.0:                   # hi == lo on the general branch: a varying smooth vector with zero span
        smooth = (0.0, 0.5, -0.5)
    th["smooth"] = np.array(smooth)
    sl = (nu, nu)
    fit = _fit(locs, X, z, sl)
    try:
        info, _ = fit.fisher_core(th, UNITS)
    finally:
        fit.close()
    assert np.all(info[12:15] == 0.0) and np.all(info[:, 12:15] == 0.0)
    R, _ = _reference(n, "units", sl, smooth)
    assert np.all(R[12:15] == 0.0)
    gap = FR.metric(info, R)
    print("nu=%g gap %.2e" % (nu, gap))
    assert gap <= TOL


def _raw_call(fit, th, dirs, with_mean=True):
    from cocons_amd.host import _p, theta_table
    T = theta_table(th)
    D = np.ascontiguousarray(np.asarray(dirs, float).reshape(-1, 18))
    nd = D.shape[0]
    info, im = np.full((nd, nd), 7.0), np.full((3, 3), 7.0)
    rc = fit._L.cocons_fisher_dense(fit._h, _p(T), nd, _p(D), _p(info), _p(im) if with_mean else None)
    return rc, info, im


def test_handle_behaviour_repeats_neighbours_failing_minor_krige():
    """two calls agree bit for bit; a value call, a gradient call and the krige state give the same bits before and after;
    a failing minor returns its index and writes nothing; info_mean may be NULL; non-finite directions are refused"""
    from cocons_amd import _lib, workloads as wl
    n = 1000
    locs, X, th, z = _setup(n, 1)
    dirs = _mixes()[:3]
    fit = _fit(locs, X, z)
    try:
        fit.krige_prepare(th)
        lp = np.random.default_rng(1).uniform(0, 1, size=(200, 2))
        Xp = wl.design_from_locs(lp)["std.covs"]
        s0, q0 = fit.krige_core(lp, Xp)
        v0, p0 = fit.neg2loglik_core(th)
        g0 = fit.neg2loglik_grad_core(th)
        a = fit.fisher_core(th, dirs)
        b = fit.fisher_core(th, dirs)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        v1, p1 = fit.neg2loglik_core(th)
        g1 = fit.neg2loglik_grad_core(th)
        assert v1 == v0 and np.array_equal(p1, p0)
        assert g1[0] == g0[0] and all(np.array_equal(x, y) for x, y in zip(g1[1:], g0[1:]))
        # a near-constant covariance without nugget: not positive definite (test_gpu_grad's failing minor)
        bad = OrderedDict((k, np.array(v, float)) for k, v in th.items())
        bad["nugget"] = np.array([-np.inf, 0.0, 0.0])
        bad["scale"][0] = np.log(50.0)
        rc, info, im = _raw_call(fit, bad, dirs)
        assert rc > 0
        assert np.all(info == 7.0) and np.all(im == 7.0)
        with pytest.raises(_lib.CholeskyError):
            fit.fisher_core(bad, dirs)
        rc, info, im = _raw_call(fit, th, dirs, with_mean=False)
        assert rc == 0 and np.array_equal(info, a[0]) and np.all(im == 7.0)
        nf = np.array(dirs)
        nf[1, 2, 1] = np.nan
        rc, info, im = _raw_call(fit, th, nf)
        assert rc == -1 and _lib.last_error().startswith("cocons_fisher_dense:") and "non-finite" in _lib.last_error()
        assert np.all(info == 7.0) and np.all(im == 7.0)
        v2, p2 = fit.neg2loglik_core(th)
        assert v2 == v0 and np.array_equal(p2, p0)
        s1, q1 = fit.krige_core(lp, Xp)
        assert np.array_equal(s0, s1) and np.array_equal(q0, q1)
    finally:
        fit.close()


def test_zero_matrix_first_minor():
    """std.dev and nugget intercepts at -Inf: Sigma = 0, the first minor fails; nothing is written"""
    n = 130
    locs, X, th, z = _setup(n, 1)
    bad = OrderedDict((k, np.array(v, float)) for k, v in th.items())
    bad["std.dev"][0] = -np.inf
    bad["nugget"][0] = -np.inf
    fit = _fit(locs, X, z)
    try:
        rc, info, im = _raw_call(fit, bad, UNITS[:2])
        assert rc == 1 and np.all(info == 7.0) and np.all(im == 7.0)
        good = fit.fisher_core(th, UNITS[:2])
    finally:
        fit.close()
    assert np.all(np.diag(good[0]) > 0)


def test_taper_sharded_and_no_z_handles_refused():
    from cocons_amd import CoconsTaperFit, workloads as wl, _lib
    from cocons_amd.host import _f, _p, theta_table
    n = 200
    locs, X, th, z = _setup(n, 1)
    ci = np.arange(1, n + 1, dtype=np.int32)
    rp = np.arange(1, n + 2, dtype=np.int32)
    T = theta_table(th)
    D = np.ascontiguousarray(UNITS[:2].reshape(2, 18))
    info, im = np.full(4, 7.0), np.full(9, 7.0)
    tf = CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, np.ones(n))
    try:
        assert tf._L.cocons_fisher_dense(tf._h, _p(T), 2, _p(D), _p(info), _p(im)) == -1
        assert _lib.last_error().startswith("cocons_fisher_dense:")
    finally:
        tf.close()
    fit = _fit(locs, X, z)
    try:
        L = fit._L
        noop_b = _lib.BCAST_FN(lambda *a: 0)
        noop_r = _lib.ALLREDUCE_FN(lambda *a: 0)
        assert L.cocons_fit_set_collectives(fit._h, 0, 2, ctypes.cast(noop_b, ctypes.c_void_p),
                                            ctypes.cast(noop_r, ctypes.c_void_p), None) == 0
        assert L.cocons_fisher_dense(fit._h, _p(T), 2, _p(D), _p(info), _p(im)) == -1
        assert _lib.last_error().startswith("cocons_fisher_dense:") and "sharded" in _lib.last_error()
    finally:
        fit.close()
    L = _lib.load()
    lf, Xf, sl = _f(locs), _f(X), np.array(wl.SMOOTH_LIMITS, float)
    h = L.cocons_fit_create(n, 3, 0, 0, _p(lf), _p(Xf), None, None, _p(sl), -1)
    assert h
    try:
        assert L.cocons_fisher_dense(h, _p(T), 2, _p(D), _p(info), _p(im)) == -1
        assert _lib.last_error().startswith("cocons_fisher_dense:") and "no z" in _lib.last_error()
    finally:
        L.cocons_fit_destroy(h)
    assert np.all(info == 7.0) and np.all(im == 7.0)


def test_host_getFisher_dense():
    """host.getFisher_dense on par_pos_full against the reference pushed through the same Jacobian, with and without a
    free mean"""
    from cocons_amd import host, workloads as wl
    n, r = 300, 2
    locs, X, th, z = _setup(n, r, coincident=True)
    R, Rm = _reference(n, "units")
    It = r * np.asarray(R).reshape(18, 18)
    fit = _fit(locs, X, z)
    try:
        for free_mean in (False, True):
            pp = wl.par_pos_full()
            tl = OrderedDict((k, np.array(v, float)) for k, v in th.items())
            if free_mean:
                pp["mean"] = [True] * 3
            else:
                tl["mean"] = np.zeros(3)
            x0 = wl.theta_vector_from_lists(tl, pp)
            got = host.getFisher_dense(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, fit=fit)
            want = host.fisher_to_par(It, r * np.asarray(Rm), x0, pp)
            assert got.shape == (x0.size, x0.size)
            gap = FR.metric(got, want)
            print("free mean %s: P = %d gap %.2e" % (free_mean, x0.size, gap))
            assert gap <= TOL
            assert np.linalg.eigvalsh(got)[0] > 0
            if free_mean:
                assert np.all(got[:3, 3:] == 0) and np.all(got[3:, :3] == 0)
    finally:
        fit.close()
