"""Expected (Fisher) information of a tapered fit on the band factor (cocons_fisher_taper) on the GPU: exact mode against the
numpy / scipy statement (tests/fisher_taper_reference.py), probe mode against the same sweep in numpy with the same probes,
orthogonal probes against the exact mode, the scaling identity, linearity, fixed smoothness, bit-identical repeats / chunk
sizes / buffer layouts, the handle's other entries before and after, a failing minor, the refusals that need a handle, the host
entry getFisher_sparse and the R glue.  Metric and bound are those of tests/test_gpu_fisher.py."""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_taper_reference as FT  # noqa: E402
from test_gpu_parity import _problem, _taper_pattern  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-7          # tests/test_gpu_fisher.py


def _dirs():
    """the nine unit entries of the std.dev, scale and smooth rows, the nugget intercept, v_s and a seeded mix over all six
    rows (the aniso and tilt rows do not enter the taper model)"""
    std = FT.standard_directions(3)
    mix = np.random.default_rng(41).standard_normal((6, 3))
    return np.concatenate([std, mix[None]])


V_S = 10            # index of v_s in _dirs()


def _setup(n, r, delta, grid=None):
    from cocons_amd import workloads as wl
    if grid:
        gx, gy = grid
        assert gx * gy == n
        cx, cy = (np.arange(gx) + 0.5) / gx, (np.arange(gy) + 0.5) / gy
        locs = np.column_stack([np.tile(cx, gy), np.repeat(cy, gx)])
        X = wl.design_from_locs(locs)["std.covs"]
        th = wl.theta_full(scale0=np.log(0.2))
        rng = np.random.default_rng(n)
    else:
        locs, X, th, rng = _problem(n, seed=900 + n)
    th["mean"] = np.array([0.3, -0.2, 0.1])
    z = rng.standard_normal((n, r))
    return locs, X, th, z, _taper_pattern(locs, delta)


def _fit(locs, X, z, ref_taper, sl=None):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    return ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS if sl is None else sl, *ref_taper)


@functools.lru_cache(maxsize=None)
def _reference(n, delta, sl=None, smooth=None):
    """(S, S_a, I at r = 1, X' S^-1 X) for _dirs() on _setup(n, ., delta): computed once, left unchanged"""
    from cocons_amd import host, workloads as wl
    locs, X, th, _, ref = _setup(n, 1, delta)
    if smooth is not None:
        th["smooth"] = np.array(smooth)
    S, Sa = FT.direction_matrices(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS if sl is None else sl, ref, _dirs())
    out = (S, Sa, FT.info_whiten(S, Sa, 1), FT.info_mean(S, X, 1))
    for a in out:
        a.setflags(write=False)
    return out


def _band(fit):
    info = fit.krige_taper_info()
    return info["W"], info["nt"]


@pytest.mark.parametrize("n,r,delta,max_rows", [(150, 1, 0.25, 0), (700, 2, 0.25, 0), (1500, 1, 0.12, 64)])
def test_exact_mode_against_reference(n, r, delta, max_rows):
    """two tile columns; six; twelve with a band narrower than the matrix and 24 chunks"""
    locs, X, th, z, ref = _setup(n, r, delta)
    fit = _fit(locs, X, z, ref)
    try:
        W, nt = _band(fit)
        info, info_mean = fit.fisher_core(th, _dirs(), max_rows=max_rows)
    finally:
        fit.close()
    if n == 1500:
        assert W < nt, (W, nt)
    _, _, R, Rm = _reference(n, delta)
    gap = FT.metric(info, r * R)
    gm = np.max(np.abs(info_mean - r * Rm)) / np.max(np.abs(Rm * r))
    print("n=%d r=%d W=%d nt=%d exact mode gap %.2e, info_mean %.2e" % (n, r, W, nt, gap, gm))
    assert gap <= TOL
    assert gm <= 1e-10
    assert np.array_equal(info, info.T) and np.array_equal(info_mean, info_mean.T)


@pytest.mark.parametrize("nprobe", [64, 100])
def test_probe_mode_against_the_numpy_sweep(nprobe):
    """the caller's probes through the handle's own order: the same probes through fisher_taper_reference.band_fisher with
    the handle's pivot; 100 probes leave the second strip partly filled"""
    n, r, delta = 700, 2, 0.25
    locs, X, th, z, ref = _setup(n, r, delta)
    P = np.random.default_rng(nprobe).integers(0, 2, size=(n, nprobe)) * 2.0 - 1.0
    fit = _fit(locs, X, z, ref)
    try:
        pivot = fit.order()
        info, info_mean = fit.fisher_core(th, _dirs(), probes=P)
    finally:
        fit.close()
    S, Sa, R, Rm = _reference(n, delta)
    want, wm, _, _ = FT.band_fisher(S, Sa, P, pivot, r=r, X=X)
    gap = FT.metric(info, want)
    print("nprobe=%d gap to the numpy sweep %.2e; to the exact value %.4f" % (nprobe, gap, FT.metric(info, r * R)))
    assert gap <= TOL
    assert np.max(np.abs(info_mean - r * Rm)) <= 1e-10 * np.max(np.abs(r * Rm))     # exact in probe mode too
    assert np.array_equal(info, info.T)


def test_orthogonal_probes_equal_the_exact_mode():
    """sqrt(n) Q, Q orthogonal, nprobe = n = 300: sum_k e_k e_k' = n I, the dense-probe path end to end"""
    from scipy import linalg
    n, delta = 300, 0.25
    locs, X, th, z, ref = _setup(n, 1, delta)
    Q = linalg.qr(np.random.default_rng(2).standard_normal((n, n)))[0]
    fit = _fit(locs, X, z, ref)
    try:
        exact, em = fit.fisher_core(th, _dirs())
        got, gm = fit.fisher_core(th, _dirs(), probes=np.sqrt(n) * Q)
    finally:
        fit.close()
    gap = FT.metric(got, exact)
    print("orthogonal probes against the exact mode %.2e" % gap)
    assert gap <= TOL
    assert np.array_equal(gm, em)


@pytest.mark.parametrize("n,r,delta,grid,tol", [(1500, 2, 0.12, None, 1e-9), (4000, 1, 0.06, (80, 50), 1e-8)])
def test_scaling_identity_and_linearity(n, r, delta, grid, tol):
    """I(v_s, v_s) = r n / 2 (S_{v_s} = S) without a reference; 4000 sites on an 80 x 50 grid are 32 tile columns.  The row of
    alpha v_1 + beta v_2 is alpha row 1 + beta row 2."""
    locs, X, th, z, ref = _setup(n, r, delta, grid)
    d = _dirs()
    al, be = 0.7, -1.3
    V = np.concatenate([d, (al * d[1] + be * d[4])[None], (al * d[6] + be * d[11])[None]])
    fit = _fit(locs, X, z, ref)
    try:
        info, _ = fit.fisher_core(th, V)
    finally:
        fit.close()
    print("n=%d r=%d I(v_s, v_s) - r n / 2 = %.2e" % (n, r, info[V_S, V_S] - r * n / 2))
    assert abs(info[V_S, V_S] - r * n / 2) <= tol * r * n / 2
    A = np.eye(V.shape[0])[:, :d.shape[0]]
    A[d.shape[0], [1, 4]] = al, be
    A[d.shape[0] + 1, [6, 11]] = al, be
    want = A @ info[:d.shape[0], :d.shape[0]] @ A.T
    gap = FT.metric(info, want)
    print("n=%d linearity gap %.2e" % (n, gap))
    assert gap <= 1e-10
    assert np.array_equal(info, info.T)


@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, 1.0])
def test_fixed_smoothness(nu):
    n, delta = 300, 0.25
    smooth = (0.0, 0.5, -0.5) if nu == 1.0 else (0.0, 0.0, 0.0)      # nu = 1: the Bessel branch with a zero span
    sl = (nu, nu)
    locs, X, th, z, ref = _setup(n, 1, delta)
    th["smooth"] = np.array(smooth)
    fit = _fit(locs, X, z, ref, sl)
    try:
        info, _ = fit.fisher_core(th, _dirs())
    finally:
        fit.close()
    assert np.all(info[6:9] == 0.0) and np.all(info[:, 6:9] == 0.0)
    _, _, R, _ = _reference(n, delta, sl, smooth)
    assert np.all(R[6:9] == 0.0)
    gap = FT.metric(info, R)
    print("nu=%g gap %.2e" % (nu, gap))
    assert gap <= TOL


def test_bits_repeats_chunks_and_buffer_layouts(monkeypatch):
    """two calls, max_rows = 64 / 128 / default, exact and probed, and the three buffer layouts of the handle give
    identical bits; info is symmetric to the bit and positive semi-definite"""
    n, delta = 1500, 0.12
    locs, X, th, z, ref = _setup(n, 1, delta)
    P = np.random.default_rng(8).integers(0, 2, size=(n, 200)) * 2.0 - 1.0
    res = {}
    for name, env in (("default", {}), ("unpacked", {"COCONS_TAPER_PACKED": "0"}), ("noband", {"COCONS_TAPER_BAND": "0"})):
        for k in ("COCONS_TAPER_PACKED", "COCONS_TAPER_BAND"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        fit = _fit(locs, X, z, ref)
        try:
            W, nt = _band(fit)
            assert (W == nt) if name == "noband" else (W < nt)
            res[name] = fit.fisher_core(th, _dirs()) + fit.fisher_core(th, _dirs(), probes=P)
            if name == "default":
                again = fit.fisher_core(th, _dirs()) + fit.fisher_core(th, _dirs(), probes=P)
                assert all(np.array_equal(a, b) for a, b in zip(again, res[name]))
                for max_rows in (64, 128):
                    got = fit.fisher_core(th, _dirs(), max_rows=max_rows) + fit.fisher_core(th, _dirs(), probes=P, max_rows=max_rows)
                    assert all(np.array_equal(a, b) for a, b in zip(got, res[name])), max_rows
        finally:
            fit.close()
    for name in ("unpacked", "noband"):
        assert all(np.array_equal(a, b) for a, b in zip(res[name], res["default"])), name
    for info in (res["default"][0], res["default"][2]):
        assert np.array_equal(info, info.T)
        ev = np.linalg.eigvalsh(info)
        print("smallest eigenvalue %.3e of trace %.3e" % (ev[0], np.trace(info)))
        assert ev[0] >= -1e-12 * np.trace(info)


def _raw_call(fit, th, dirs, probes=None, max_rows=0, with_mean=True):
    from cocons_amd.host import _f, _p, theta_table
    T = theta_table(th)
    D = np.ascontiguousarray(np.asarray(dirs, float).reshape(-1, 18))
    nd = D.shape[0]
    info, im = np.full((nd, nd), 7.0), np.full((3, 3), 7.0)
    Pm = None if probes is None else _f(probes)
    rc = fit._L.cocons_fisher_taper(fit._h, _p(T), nd, _p(D), 0 if Pm is None else Pm.shape[1], None if Pm is None else _p(Pm),
                                    max_rows, _p(info), _p(im) if with_mean else None)
    return rc, info, im


def test_the_handle_before_and_after_failing_minor_and_refusals():
    """value, gradient, leave-one-out and a prepared kriging state give the same bits before and after Fisher calls; a theta
    with a non-positive pivot returns the minor, writes nothing, and the next call succeeds; info_mean may be NULL;
    non-finite directions and probes and a dense handle are refused"""
    from cocons_amd import CoconsFit, _lib, workloads as wl
    n, delta = 900, 0.15
    locs, X, th, z, ref = _setup(n, 2, delta)
    dirs = _dirs()[[0, 4, 8, 9]]
    rng = np.random.default_rng(1)
    lp = rng.uniform(0.05, 0.95, size=(150, 2))
    Xp = wl.design_from_locs(lp)["std.covs"]
    from test_gpu_parity import _csr_within, _wendland1
    pci, prp = _csr_within(lp, locs, delta)
    pent = np.empty(pci.size)
    for i in range(lp.shape[0]):
        w0, w1 = prp[i] - 1, prp[i + 1] - 1
        pent[w0:w1] = _wendland1(np.sqrt(np.sum((locs[pci[w0:w1] - 1] - lp[i]) ** 2, axis=1)), delta)
    pt = (pci, prp, pent)
    P = rng.integers(0, 2, size=(n, 64)) * 2.0 - 1.0
    fit = _fit(locs, X, z, ref)
    try:
        fit.krige_taper_prepare(th, max_rows=128)
        k0 = fit.krige_taper_core(lp, Xp, pt)
        v0 = fit.neg2loglik_core(th)
        g0 = fit.neg2loglik_grad_core(th)
        c0 = fit.cv_core(th)
        a = fit.fisher_core(th, dirs)
        b = fit.fisher_core(th, dirs, probes=P)
        v1, g1, c1, k1 = fit.neg2loglik_core(th), fit.neg2loglik_grad_core(th), fit.cv_core(th), fit.krige_taper_core(lp, Xp, pt)
        assert v1[0] == v0[0] and np.array_equal(v1[1], v0[1])
        assert g1[0] == g0[0] and all(np.array_equal(x, y) for x, y in zip(g1[1:], g0[1:]))
        assert all(np.array_equal(x, y) for x, y in zip(c1, c0)) and all(np.array_equal(x, y) for x, y in zip(k1, k0))
        bad = OrderedDict((k, np.array(v, float)) for k, v in th.items())
        bad["std.dev"][0] = -np.inf
        bad["nugget"][0] = -np.inf
        for pr in (None, P):
            rc, info, im = _raw_call(fit, bad, dirs, pr)
            assert rc == 1 and np.all(info == 7.0) and np.all(im == 7.0)
        with pytest.raises(_lib.CholeskyError):
            fit.fisher_core(bad, dirs)
        rc, info, im = _raw_call(fit, th, dirs, with_mean=False)
        assert rc == 0 and np.array_equal(info, a[0]) and np.all(im == 7.0)
        rc, info, im = _raw_call(fit, th, dirs, P)
        assert rc == 0 and np.array_equal(info, b[0]) and np.array_equal(im, a[1])
        nf = np.array(dirs)
        nf[1, 0, 1] = np.nan
        rc, info, im = _raw_call(fit, th, nf)
        assert rc == -1 and _lib.last_error().startswith("cocons_fisher_taper:") and "non-finite" in _lib.last_error()
        Pn = P.copy()
        Pn[5, 3] = np.inf
        rc, info, im = _raw_call(fit, th, dirs, Pn)
        assert rc == -1 and _lib.last_error().startswith("cocons_fisher_taper:") and "non-finite" in _lib.last_error()
        assert np.all(info == 7.0) and np.all(im == 7.0)
        k2 = fit.krige_taper_core(lp, Xp, pt)
        assert all(np.array_equal(x, y) for x, y in zip(k2, k0))
    finally:
        fit.close()
    dense = CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        rc, info, im = _raw_call(dense, th, dirs)
        assert rc == -1 and _lib.last_error().startswith("cocons_fisher_taper:") and "taper" in _lib.last_error()
        assert np.all(info == 7.0) and np.all(im == 7.0)
    finally:
        dense.close()


def test_host_getFisher_sparse_and_glue():
    """host.getFisher_sparse on par_pos_full (aniso and tilt free: zero rows) against the reference pushed through the same
    Jacobian, with and without a free mean, exact and probed; the R glue returns fisher_core's bits"""
    from cocons_amd import host, workloads as wl
    from test_glue_exec import RStub
    n, r, delta = 700, 2, 0.25
    locs, X, th, z, ref = _setup(n, r, delta)
    units = np.eye(18).reshape(18, 6, 3)
    S, Sa = FT.direction_matrices(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, ref, units)
    It, Rm = FT.info_whiten(S, Sa, r), FT.info_mean(S, X, r)
    fit = _fit(locs, X, z, ref)
    try:
        for free_mean in (False, True):
            pp = wl.par_pos_full()
            tl = OrderedDict((k, np.array(v, float)) for k, v in th.items())
            if free_mean:
                pp["mean"] = [True] * 3
            else:
                tl["mean"] = np.zeros(3)
            x0 = wl.theta_vector_from_lists(tl, pp)
            got = host.getFisher_sparse(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, ref, fit=fit)
            want = host.fisher_to_par(It, Rm, x0, pp)
            gap = FT.metric(got, want)
            print("free mean %s: P = %d gap %.2e" % (free_mean, x0.size, gap))
            assert got.shape == (x0.size, x0.size) and gap <= TOL
            est = host.getFisher_sparse(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, ref, nprobe=64, seed=3, fit=fit)
            assert np.array_equal(est, host.getFisher_sparse(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, ref, nprobe=64, seed=3, fit=fit))
            print("64 probes against the exact value %.4f" % FT.metric(est, want))      # (the accuracy a user gets: not asserted)
            assert np.array_equal(est, est.T) and np.linalg.eigvalsh(est)[0] >= -1e-12 * np.trace(est)
        dirs = _dirs()
        P = np.random.default_rng(4).integers(0, 2, size=(n, 70)) * 2.0 - 1.0
        a = fit.fisher_core(th, dirs, max_rows=64)
        b = fit.fisher_core(th, dirs, probes=P)
    finally:
        fit.close()
    R = RStub()
    ci, rp, ent = ref
    h = R.call("_cocons_hip_fit_create_taper", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer(ci), R.integer(rp), R.real(ent))
    D = np.ascontiguousarray(dirs.reshape(-1, 18).T)
    st, res = R.value(R.call("_cocons_hip_fisher_taper", h, R.theta(th), R.real(D), R.nil, R.integer([64])))
    assert int(st[0]) == 0 and np.array_equal(res[0], a[0]) and np.array_equal(res[1], a[1])
    st, res = R.value(R.call("_cocons_hip_fisher_taper", h, R.theta(th), R.real(D), R.real(P), R.integer([0])))
    assert int(st[0]) == 0 and np.array_equal(res[0], b[0]) and np.array_equal(res[1], b[1])
    R.L.stub_gc(0, None)
