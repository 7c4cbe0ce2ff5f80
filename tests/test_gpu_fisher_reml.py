"""Expected information of the REML fit on the GPU (cocons_fisher_reml): against the numpy / scipy statement
(tests/fisher_reml_reference.py, the projector form) in the metric of tests/fisher_reference.py, a border that crosses a
128-tile, the exact identity I_R(v_s, v_s) = r (n - 3) / 2, symmetry and positive semi-definiteness, linearity in the
directions, fixed smoothness, bit-identical repeats, the handle's other entries before and after, failing minors, a design
whose W = X' Sigma^-1 X is not positive definite, refusals and the host entry getFisher_reml."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
import fisher_reml_reference as RR  # noqa: E402
from test_gpu_fisher import TOL, UNITS, _fit, _mixes, _setup  # noqa: E402

pytestmark = pytest.mark.gpu

WHO = "cocons_fisher_reml:"


@functools.lru_cache(maxsize=None)
def _reference(n, kind, sl=None, smooth=None):
    """I_R at r = 1 of the n-site problem for the 18 unit directions (kind 'units') or the 7 mixes ('mixes'), by the
    projector form; computed once and left unchanged"""
    from cocons_amd import host, workloads as wl
    locs, X, th, _ = _setup(n, 1, coincident=(n == 300))
    if smooth is not None:
        th["smooth"] = np.array(smooth)
    limits = wl.SMOOTH_LIMITS if sl is None else sl
    S, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, limits, UNITS if kind == "units" else _mixes())
    I = RR.info_projector(S, Sa, X, 1)
    I.setflags(write=False)
    return I


def _raw_call(fit, th, dirs):
    from cocons_amd.host import _p, theta_table
    T = theta_table(th)
    D = np.ascontiguousarray(np.asarray(dirs, float).reshape(-1, 18))
    nd = D.shape[0]
    info = np.full((nd, nd), 7.0)
    rc = fit._L.cocons_fisher_reml(fit._h, _p(T), nd, _p(D), _p(info))
    return rc, info


@pytest.mark.parametrize("n,r", [(300, 1), (300, 3), (130, 1)])
def test_unit_directions_against_reference(n, r):
    locs, X, th, z = _setup(n, r, coincident=(n == 300))
    fit = _fit(locs, X, z)
    try:
        info = fit.fisher_reml_core(th, UNITS)
    finally:
        fit.close()
    gap = FR.metric(info, r * _reference(n, "units"))
    print("n=%d r=%d gap %.2e" % (n, r, gap))
    assert gap <= TOL
    assert np.array_equal(info, info.T)


def test_wide_border_r126():
    """[Z' ; X' ; I] has 126 + 3 = 129 rows in front of the unit rows: two tile rows, the wider leading dimension"""
    n, r = 300, 126
    locs, X, th, z = _setup(n, r, coincident=True)
    fit = _fit(locs, X, z)
    try:
        info = fit.fisher_reml_core(th, UNITS)
    finally:
        fit.close()
    gap = FR.metric(info, r * _reference(n, "units"))
    print("n=%d r=%d gap %.2e" % (n, r, gap))
    assert gap <= TOL
    assert np.array_equal(info, info.T)


def test_mixed_directions_against_reference_n2116():
    """17 tiles of 128: crosses the 256-column blocks of the factorisation and the column panels of the products"""
    n = 2116
    locs, X, th, z = _setup(n, 1)
    fit = _fit(locs, X, z)
    try:
        info = fit.fisher_reml_core(th, _mixes())
    finally:
        fit.close()
    gap = FR.metric(info, _reference(n, "mixes"))
    print("n=%d gap %.2e; I_R(v_s, v_s) - (n - 3) / 2 = %.2e" % (n, gap, info[0, 0] - (n - 3) / 2))
    assert gap <= TOL
    assert abs(info[0, 0] - (n - 3) / 2) <= 1e-9 * n


def test_identities():
    """no reference needed: I_R(v_s, v_s) = r (n - 3) / 2 (P Sigma P = P, tr(P Sigma) = n - rank X), symmetry to the bit,
    positive semi-definiteness"""
    n, r = 2116, 3
    locs, X, th, z = _setup(n, r, seed=9)
    fit = _fit(locs, X, z)
    try:
        info = fit.fisher_reml_core(th, _mixes())
    finally:
        fit.close()
    print("n=%d r=%d I_R(v_s, v_s) - r (n - 3) / 2 = %.2e" % (n, r, info[0, 0] - r * (n - 3) / 2))
    assert abs(info[0, 0] - r * (n - 3) / 2) <= 1e-9 * n
    assert np.array_equal(info, info.T)
    d = np.sqrt(np.diag(info))
    assert np.all(d > 0)
    lam = np.linalg.eigvalsh(info / np.outer(d, d))[0]
    print("smallest eigenvalue of the normalised matrix %.3e" % lam)
    assert lam >= -1e-10


def test_direction_linearity():
    """the row of 0.5 (e_a + e_b) is 0.5 (row a + row b): pairs across scale k = 0 / k >= 1 and across families"""
    n = 300
    locs, X, th, z = _setup(n, 1, coincident=True)
    flat = np.eye(18)
    pairs = [(3, 4), (3, 5), (4, 5), (0, 3), (0, 4), (15, 1), (12, 9)]       # (t * 3 + k)
    V = np.concatenate([flat, np.stack([0.5 * (flat[a] + flat[b]) for a, b in pairs])])
    fit = _fit(locs, X, z)
    try:
        info = fit.fisher_reml_core(th, V)
    finally:
        fit.close()
    want = V @ info[:18, :18] @ V.T
    gap = FR.metric(info, want)
    print("linearity gap %.2e" % gap)
    assert gap <= 1e-12


@pytest.mark.parametrize("nu", [0.5, 1.5])
def test_fixed_smoothness(nu):
    n = 300
    locs, X, th, z = _setup(n, 1, coincident=True)
    smooth = (0.0, 0.0, 0.0)
    th["smooth"] = np.array(smooth)
    sl = (nu, nu)
    fit = _fit(locs, X, z, sl)
    try:
        info = fit.fisher_reml_core(th, UNITS)
    finally:
        fit.close()
    assert np.all(info[12:15] == 0.0) and np.all(info[:, 12:15] == 0.0)
    R = _reference(n, "units", sl, smooth)
    assert np.all(R[12:15] == 0.0)
    gap = FR.metric(info, R)
    print("nu=%g gap %.2e" % (nu, gap))
    assert gap <= TOL


def test_handle_behaviour_repeats_neighbours_failing_minor_krige():
    """two calls agree bit for bit; the value, the dense and REML gradients, the dense information and the krige state give
    the same bits before and after; a failing minor returns its index and writes nothing; non-finite directions are refused"""
    from cocons_amd import _lib, workloads as wl
    n = 1000
    locs, X, th, z = _setup(n, 1)
    dirs = _mixes()[:3]
    fit = _fit(locs, X, z)
    try:
        fit.krige_prepare(th)
        lp = np.random.default_rng(1).uniform(0, 1, size=(200, 2))
        Xp = wl.design_from_locs(lp)["std.covs"]

        def neighbours():
            v, p = fit.neg2loglik_core(th)
            out = [np.array([v]), p]
            out += [np.atleast_1d(x) for x in fit.neg2loglik_grad_core(th)]
            out += [np.atleast_1d(x) for x in fit.neg2loglik_reml_grad_core(th, 3)]
            out += list(fit.fisher_core(th, dirs))
            out += list(fit.krige_core(lp, Xp))
            return out

        before = neighbours()
        a = fit.fisher_reml_core(th, dirs)
        b = fit.fisher_reml_core(th, dirs)
        assert np.array_equal(a, b) and np.array_equal(a, a.T)
        after = neighbours()
        assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
        # a near-constant covariance without nugget: not positive definite (test_gpu_grad's failing minor)
        bad = OrderedDict((k, np.array(v, float)) for k, v in th.items())
        bad["nugget"] = np.array([-np.inf, 0.0, 0.0])
        bad["scale"][0] = np.log(50.0)
        rc, info = _raw_call(fit, bad, dirs)
        assert rc > 0
        assert np.all(info == 7.0)
        with pytest.raises(_lib.CholeskyError):
            fit.fisher_reml_core(bad, dirs)
        nf = np.array(dirs)
        nf[1, 2, 1] = np.nan
        rc, info = _raw_call(fit, th, nf)
        assert rc == -1 and _lib.last_error().startswith(WHO) and "non-finite" in _lib.last_error()
        assert np.all(info == 7.0)
        rc, info = _raw_call(fit, th, dirs)
        assert rc == 0 and np.array_equal(info, a)
        again = neighbours()
        assert all(np.array_equal(x, y) for x, y in zip(before, again))
    finally:
        fit.close()


def test_w_not_positive_definite():
    """a design whose last column is all zeros: a pivot of W = X' Sigma^-1 X is exactly 0.  -4, the entry's name, info
    untouched -- never the ML information, which the zeroed low-rank block would give --; the dense entry still serves the
    handle"""
    from cocons_amd import _lib
    n = 300
    locs, X, th, z = _setup(n, 1, coincident=True)
    X = np.array(X)
    X[:, 2] = 0.0
    fit = _fit(locs, X, z)
    try:
        rc, info = _raw_call(fit, th, UNITS[:2])
        assert rc == -4, (rc, _lib.last_error())
        assert _lib.last_error().startswith(WHO) and "positive definite" in _lib.last_error()
        assert np.all(info == 7.0)
        dense, _ = fit.fisher_core(th, UNITS[:2])
    finally:
        fit.close()
    assert np.all(np.diag(dense) > 0)


def test_taper_sharded_and_no_z_handles_refused():
    from cocons_amd import CoconsTaperFit, workloads as wl, _lib
    from cocons_amd.host import _f, _p, theta_table
    n = 200
    locs, X, th, z = _setup(n, 1)
    ci = np.arange(1, n + 1, dtype=np.int32)
    rp = np.arange(1, n + 2, dtype=np.int32)
    T = theta_table(th)
    D = np.ascontiguousarray(UNITS[:2].reshape(2, 18))
    info = np.full(4, 7.0)
    tf = CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, np.ones(n))
    try:
        assert tf._L.cocons_fisher_reml(tf._h, _p(T), 2, _p(D), _p(info)) == -1
        assert _lib.last_error().startswith(WHO)
    finally:
        tf.close()
    fit = _fit(locs, X, z)
    try:
        L = fit._L
        noop_b = _lib.BCAST_FN(lambda *a: 0)
        noop_r = _lib.ALLREDUCE_FN(lambda *a: 0)
        assert L.cocons_fit_set_collectives(fit._h, 0, 2, ctypes.cast(noop_b, ctypes.c_void_p),
                                            ctypes.cast(noop_r, ctypes.c_void_p), None) == 0
        assert L.cocons_fisher_reml(fit._h, _p(T), 2, _p(D), _p(info)) == -1
        assert _lib.last_error().startswith(WHO) and "sharded" in _lib.last_error()
    finally:
        fit.close()
    L = _lib.load()
    lf, Xf, sl = _f(locs), _f(X), np.array(wl.SMOOTH_LIMITS, float)
    h = L.cocons_fit_create(n, 3, 0, 0, _p(lf), _p(Xf), None, None, _p(sl), -1)
    assert h
    try:
        assert L.cocons_fisher_reml(h, _p(T), 2, _p(D), _p(info)) == -1
        assert _lib.last_error().startswith(WHO) and "no z" in _lib.last_error()
    finally:
        L.cocons_fit_destroy(h)
    assert np.all(info == 7.0)


def test_host_getFisher_reml():
    """host.getFisher_reml on par_pos_full (no free mean) against J_t (r I_R) J_t' built from the reference; a free mean
    raises ValueError"""
    from cocons_amd import host, workloads as wl
    n, r = 300, 2
    locs, X, th, z = _setup(n, r, coincident=True)
    It = r * np.asarray(_reference(n, "units")).reshape(18, 18)
    fit = _fit(locs, X, z)
    try:
        pp = wl.par_pos_full()
        tl = OrderedDict((k, np.array(v, float)) for k, v in th.items())
        tl["mean"] = np.zeros(3)
        x0 = wl.theta_vector_from_lists(tl, pp)
        got = host.getFisher_reml(x0, pp, locs, X, None, wl.SMOOTH_LIMITS, z, n, fit=fit)
        Jt, Jm = host.fisher_jacobian(x0, pp)
        assert not np.any(Jm)
        want = Jt @ It @ Jt.T
        assert got.shape == (x0.size, x0.size)
        gap = FR.metric(got, want)
        lam = np.linalg.eigvalsh(got)[0]
        print("P = %d gap %.2e smallest eigenvalue %.3e" % (x0.size, gap, lam))
        assert gap <= TOL
        assert lam > 0
        pp["mean"] = [True] * 3
        x1 = wl.theta_vector_from_lists(th, pp)
        with pytest.raises(ValueError):
            host.getFisher_reml(x1, pp, locs, X, None, wl.SMOOTH_LIMITS, z, n, fit=fit)
    finally:
        fit.close()
