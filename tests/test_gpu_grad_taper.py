"""cocons_neg2loglik_grad_taper (the tapered -2 log-likelihood and its analytic gradient through the selected inverse on the
band factor's tile envelope) and its diagnostic cocons_debug_taper_selinv on the GPU, against

  * tests/grad_taper_reference.py (dense inverse of the assembled matrix; pinned to the CPU oracle by
    tests/test_grad_taper_reference.py),
  * numpy.linalg.inv / scipy.sparse.linalg.splu of the oracle's matrix,
  * the scaling identity  df/dsd_0 + df/dnugget_0 = r n - sum of the quadratic forms  (T is fixed),
  * Richardson differences of the library's own value entry.

Sizes and taper ranges are those of test_taper_objective_vs_oracle (two tiles, several tiles, band-limited packed buffer);
the tolerances are the dense gradient's (tests/test_gpu_grad.py)."""
import ctypes
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_taper_reference as GT  # noqa: E402
from test_gpu_parity import _problem, _taper_pattern  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(150, 1), (700, 2), (1500, 1), (4000, 1)]


def _delta(n):
    return 0.25 if n < 1000 else (0.12 if n < 3000 else 0.06)      # as test_taper_objective_vs_oracle


def _inf(a):
    return float(np.max(np.abs(a)))


def _setup(n, r, seed=None):
    locs, X, th, rng = _problem(n, seed=900 + n if seed is None else seed)
    th["mean"] = np.array([0.3, -0.2, 0.1])
    z = rng.standard_normal((n, r))
    return locs, X, th, z, rng


def _taper_fit(locs, X, z, ref_taper):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    return ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)


def _selinv(fit, th, nnz):
    from cocons_amd.host import _p, theta_table
    out = np.full(nnz, np.nan)
    nbytes = ctypes.c_longlong(-1)
    rc = fit._L.cocons_debug_taper_selinv(fit._h, _p(theta_table(th)), _p(out), ctypes.byref(nbytes))
    assert rc == 0, rc
    return out, nbytes.value


def _fit_memory(fit):
    out = (ctypes.c_longlong * 4)()
    assert fit._L.cocons_debug_fit_memory(fit._h, out) == 0
    return list(out)


@pytest.mark.parametrize("n,r", SIZES)
def test_value_and_gradient_vs_reference(n, r):
    """Value and parts equal the value entry's on the same handle (1e-12); grad_theta, grad_quad and grad_mean against the
    numpy statement (1e-7 of each one's largest component); the scaling identity (1e-9 r n); two calls give identical bits;
    value calls before and after are bit-identical."""
    from cocons_amd import workloads as wl
    locs, X, th, z, _ = _setup(n, r)
    ref_taper = _taper_pattern(locs, _delta(n))
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        v0, p0 = fit.neg2loglik_core(th)
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(th)
        v1, p1 = fit.neg2loglik_core(th)
        again = fit.neg2loglik_grad_core(th)
    finally:
        fit.close()
    assert v1 == v0 and np.array_equal(p1, p0)
    print("n=%d value rel %.3e, parts rel %.3e" % (n, abs(v - v0) / abs(v0), _inf(parts - p0) / _inf(p0)))
    assert abs(v - v0) <= 1e-12 * abs(v0)
    assert _inf(parts - p0) <= 1e-12 * _inf(p0)
    assert again[0] == v and all(np.array_equal(a, b) for a, b in zip(again[1:], (parts, gt, gq, gm)))
    assert np.all(gt[2] == 0) and np.all(gt[3] == 0) and np.all(gq[2] == 0) and np.all(gq[3] == 0)
    f, rparts, rl, rq, rm = GT.neg2loglik_taper_grad(fit_table(th), th["mean"], locs, X, z, wl.SMOOTH_LIMITS, ref_taper)
    for name, got, want in (("grad_theta", gt, rl + rq), ("grad_quad", gq, rq), ("grad_mean", gm, rm)):
        print("n=%d %s: %.3e of %.3e" % (n, name, _inf(got - want), _inf(want)))
        assert _inf(got - want) <= 1e-7 * _inf(want), (name, _inf(got - want), _inf(want))
    assert abs(v - f) <= 1e-9 * abs(f)
    ident = gt[0, 0] + gt[5, 0] - (r * n - float(np.sum(parts[1:])))
    print("n=%d scaling identity: %.3e of r n = %d" % (n, abs(ident), r * n))
    assert abs(ident) <= 1e-9 * r * n


@pytest.mark.parametrize("p,r", [(1, 1), (2, 3), (7, 1), (32, 3)])
def test_design_widths_against_reference(p, r):
    """p from 1 to COCONS_P_MAX = 32 covariates in every aspect (the design matrix of test_widest_design_matrix), r = 1 and 3,
    n = 300 with taper range 0.25: grad_theta, grad_quad and grad_mean against the numpy statement at the tolerances of
    test_value_and_gradient_vs_reference; a failing first minor leaves every output untouched and the next call gives the
    first call's bits."""
    from cocons_amd import workloads as wl
    from cocons_amd.host import _p, theta_table
    from test_gpu_grad import _general_problem, _zero_matrix_theta
    n = 300
    locs, X, th, z = _general_problem(n, p, r, 7100 + p)
    ref_taper = _taper_pattern(locs, 0.25)
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(th)
        bad = _zero_matrix_theta(th)
        val = ctypes.c_double(-7.0)
        outs = [np.full(k, -7.0) for k in (1 + r, 6 * p, 6 * p, p)]
        rc = fit._L.cocons_neg2loglik_grad_taper(fit._h, _p(theta_table(bad)), _p(np.ascontiguousarray(bad["mean"])),
                                                 ctypes.byref(val), *[_p(o) for o in outs])
        assert rc > 0 and val.value == -7.0 and all(np.all(o == -7.0) for o in outs)
        again = fit.neg2loglik_grad_core(th)
    finally:
        fit.close()
    assert again[0] == v and all(np.array_equal(a, b) for a, b in zip(again[1:], (parts, gt, gq, gm)))
    assert gt.shape == (6, p) and gq.shape == (6, p) and gm.shape == (p,)
    assert np.all(gt[2] == 0) and np.all(gt[3] == 0) and np.all(gq[2] == 0) and np.all(gq[3] == 0)
    f, rparts, rl, rq, rm = GT.neg2loglik_taper_grad(fit_table(th), th["mean"], locs, X, z, wl.SMOOTH_LIMITS, ref_taper)
    assert abs(v - f) <= 1e-9 * abs(f)
    for name, got, want in (("grad_theta", gt, rl + rq), ("grad_quad", gq, rq), ("grad_mean", gm, rm)):
        print("p=%d r=%d %s: %.3e of %.3e" % (p, r, name, _inf(got - want), _inf(want)))
        assert _inf(got - want) <= 1e-7 * _inf(want), (name, _inf(got - want), _inf(want))


def fit_table(th):
    from cocons_amd.host import theta_table
    return theta_table(th)


@pytest.mark.parametrize("n,r", SIZES)
def test_selected_inverse_vs_dense_inverse(oracle, n, r):
    """cocons_debug_taper_selinv against numpy.linalg.inv of the oracle's matrix at every stored entry, in the caller's
    CSR order (1e-10 of max |S^-1|); the bytes the gradient holds do not grow from the second call on and stay within the
    matrix buffer's size plus 4 doubles per stored entry (six weighted partials and two index words per LOWER entry: 3.5)
    plus 16 + r doubles per padded site (13 per-site values, S^-1 R)."""
    from cocons_amd import workloads as wl
    locs, X, th, z, _ = _setup(n, r)
    ci, rp, ent = ref_taper = _taper_pattern(locs, _delta(n))
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        got, b1 = _selinv(fit, th, ci.size)
        fit.neg2loglik_grad_core(th)
        got2, b2 = _selinv(fit, th, ci.size)
        mem = _fit_memory(fit)
    finally:
        fit.close()
    vals = ent * oracle.cov_rns_taper(th, locs, X, ci, rp, wl.SMOOTH_LIMITS)
    rows = np.repeat(np.arange(n), np.diff(rp))
    S = np.zeros((n, n))
    S[rows, ci - 1] = vals
    want = np.linalg.inv(S)[rows, ci - 1]
    print("n=%d selected inverse: %.3e of %.3e; %d bytes held" % (n, _inf(got - want), _inf(want), b1))
    assert _inf(got - want) <= 1e-10 * _inf(want)
    assert np.array_equal(got, got2) and b1 == b2 > 0
    npad = (n + 127) // 128 * 128
    assert b1 <= mem[0] + 8 * (4 * ci.size + (16 + r) * npad), (b1, mem[0])


def test_buffer_layouts_and_orders_agree(monkeypatch):
    """The dense buffer with its band used (COCONS_TAPER_PACKED=0), no envelope at all (COCONS_TAPER_BAND=0) and the caller's
    order instead of the reverse Cuthill-McKee one (COCONS_TAPER_RCM=0) give the default's gradient to 1e-10 of its largest
    component, and the same selected inverse."""
    n, r = 4000, 1
    locs, X, th, z, _ = _setup(n, r)
    ci, rp, ent = ref_taper = _taper_pattern(locs, 0.06)
    res = {}
    for name, env in (("default", {}), ("unpacked", {"COCONS_TAPER_PACKED": "0"}), ("noband", {"COCONS_TAPER_BAND": "0"}),
                      ("norcm", {"COCONS_TAPER_RCM": "0"})):
        for k in ("COCONS_TAPER_PACKED", "COCONS_TAPER_BAND", "COCONS_TAPER_RCM"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        fit = _taper_fit(locs, X, z, ref_taper)
        try:
            mem = _fit_memory(fit)
            res[name] = fit.neg2loglik_grad_core(th) + (_selinv(fit, th, ci.size)[0], mem[0])
        finally:
            fit.close()
    base = res["default"]
    assert base[6] < res["unpacked"][6]                      # the default is the packed band
    for name in ("unpacked", "noband", "norcm"):
        got = res[name]
        assert abs(got[0] - base[0]) <= 1e-12 * abs(base[0])
        for k in (2, 3, 4):
            print("%s output %d: %.3e of %.3e" % (name, k, _inf(got[k] - base[k]), _inf(base[k])))
            assert _inf(got[k] - base[k]) <= 1e-10 * _inf(base[2])
        assert _inf(got[5] - base[5]) <= 1e-10 * _inf(base[5])


def _directional(fit, th, names, d, h):
    """Richardson central difference (steps h, h / 2) of the handle's own value along d over the named table entries"""
    def val(t):
        tl = OrderedDict((k, np.array(v, dtype=float)) for k, v in th.items())
        for (k, i), di in zip(names, d):
            tl[k][i] += t * di
        return fit.neg2loglik_core(tl)[0]

    def cd(step):
        return (val(step) - val(-step)) / (2 * step)
    return (4 * cd(h / 2) - cd(h)) / 3


def test_n40000_grid_identity_splu_and_directional_differences(oracle):
    """200 x 200 grid, taper range 0.03 (packed band): the scaling identity (1e-8 r n), S^-1 at the stored entries of 8
    columns against sparse LU solves of the oracle's matrix (1e-10 of max |S^-1|), and the gradient against Richardson
    differences of the library's own value along 3 fixed random directions in (theta, mean) (1e-6 of the analytic
    directional derivative)."""
    from scipy.sparse import csc_matrix, csr_matrix
    from scipy.sparse.linalg import splu
    from cocons_amd import workloads as wl
    from test_gpu_sim_taper import _grid_pattern
    g = 200
    n, r = g * g, 1
    locs = wl.grid_locs(g)
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full(scale0=np.log(0.05))
    th["mean"] = np.array([0.3, -0.2, 0.1])
    ci, rp, ent = ref_taper = _grid_pattern(locs, 0.03)
    z = np.random.default_rng(40001).standard_normal((n, r))
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(th)
        ident = gt[0, 0] + gt[5, 0] - (r * n - float(np.sum(parts[1:])))
        print("n=40000 scaling identity: %.3e of r n = %d" % (abs(ident), r * n))
        assert abs(ident) <= 1e-8 * r * n
        zsel, _ = _selinv(fit, th, ci.size)
        names = [(k, i) for k in ("std.dev", "scale", "smooth") for i in range(3)] + [("nugget", 0)] + \
                [("mean", i) for i in range(3)]
        rows_of = {"std.dev": 0, "scale": 1, "smooth": 4, "nugget": 5}
        gvec = np.array([gm[i] if k == "mean" else gt[rows_of[k], i] for k, i in names])
        drng = np.random.default_rng(7)
        for t in range(3):
            d = drng.uniform(-1, 1, size=len(names))
            ana = float(gvec @ d)
            num = _directional(fit, th, names, d, 1e-3)
            print("direction %d: analytic %.10e, Richardson %.10e (%.2e relative)" % (t, ana, num, abs(ana - num) / abs(ana)))
            assert abs(ana - num) <= 1e-6 * abs(ana)
    finally:
        fit.close()
    vals = ent * oracle.cov_rns_taper(th, locs, X, ci, rp, wl.SMOOTH_LIMITS)
    S = csr_matrix((vals, ci - 1, rp - 1), shape=(n, n))
    # (the grid is listed row by row: S is banded as it stands, and the natural order keeps the LU inside the band)
    lu = splu(csc_matrix(S), permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    colsel = np.array([0, 137, 5000, 12345, 20100, 27777, 33333, n - 1])
    E = np.zeros((n, colsel.size))
    E[colsel, np.arange(colsel.size)] = 1.0
    Sinv_cols = lu.solve(E)
    rows = np.repeat(np.arange(n), np.diff(rp))
    scale = _inf(zsel)
    for k, c in enumerate(colsel):
        m = (ci - 1) == c
        err = _inf(zsel[m] - Sinv_cols[rows[m], k])
        print("column %d: %.3e of %.3e" % (c, err, scale))
        assert err <= 1e-10 * scale


def test_duplicated_location(monkeypatch):
    """Two observations at one location (the `u <= eps` branch: the pair's entry is the diagonal value of its row site on
    the lower triangle), default nugget.  The earlier of the two gets the larger variance, in the caller's order
    (COCONS_TAPER_RCM=0), so that S stays positive definite.  Gradient against Richardson differences of the library's own
    value over every free table entry and the mean: 1e-6 of the largest component."""
    monkeypatch.setenv("COCONS_TAPER_RCM", "0")
    n, r = 700, 1
    locs, X, th, z, _ = _setup(n, r, seed=31)
    locs[400] = locs[5]
    X[400] = X[5]
    X[5] = X[5] + [0.0, 0.5, 0.0]
    ref_taper = _taper_pattern(locs, 0.25)
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(th)
        names = [(k, i) for k in ("std.dev", "scale", "smooth", "nugget") for i in range(3)] + [("mean", i) for i in range(3)]
        rows_of = {"std.dev": 0, "scale": 1, "smooth": 4, "nugget": 5}
        ana = np.array([gm[i] if k == "mean" else gt[rows_of[k], i] for k, i in names])
        num = np.array([_directional(fit, th, names, np.eye(len(names))[t], 1e-3) for t in range(len(names))])
    finally:
        fit.close()
    print("duplicate: %.3e of %.3e" % (_inf(ana - num), _inf(num)))
    assert _inf(ana - num) <= 1e-6 * _inf(num)


def test_failing_minor_writes_nothing_and_the_handle_recovers():
    """std.dev[0] = nugget[0] = -Inf: status k > 0 and no output written; the next good gradient call, a prediction and a
    simulation on the same handle give what they gave before."""
    import cocons_amd as ca
    from cocons_amd.host import _p, theta_table
    from test_gpu_parity import _csr_within
    n, r, m = 4000, 1, 150
    locs, X, th, z, rng = _setup(n, r, seed=4300)
    ref_taper = _taper_pattern(locs, 0.06)
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = np.column_stack([np.ones(m), rng.standard_normal(m), rng.standard_normal(m)])
    cip, rpp = _csr_within(lp, locs, 0.06)
    pred_taper = (cip, rpp, np.ones(cip.size))
    E = rng.standard_normal((n, 3))
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        pred0 = fit.predict_core(th, lp, Xp, pred_taper)
        sim0 = fit.sim_core(th, E)
        first = fit.neg2loglik_grad_core(th)
        th_bad = {k: np.array(v, dtype=float).copy() for k, v in th.items()}
        th_bad["std.dev"][0] = -np.inf
        th_bad["nugget"][0] = -np.inf
        with pytest.raises(ca.CholeskyError) as ei:
            fit.neg2loglik_grad_core(th_bad)
        assert ei.value.minor > 0
        val = ctypes.c_double(-7.0)
        outs = [np.full(k, -7.0) for k in (1 + r, 18, 18, 3)]
        rc = fit._L.cocons_neg2loglik_grad_taper(fit._h, _p(theta_table(th_bad)), _p(np.ascontiguousarray(th_bad["mean"])),
                                                 ctypes.byref(val), *[_p(o) for o in outs])
        assert rc > 0 and val.value == -7.0 and all(np.all(o == -7.0) for o in outs)
        again = fit.neg2loglik_grad_core(th)
        assert again[0] == first[0] and all(np.array_equal(a, b) for a, b in zip(again[1:], first[1:]))
        pred1 = fit.predict_core(th, lp, Xp, pred_taper)
        sim1 = fit.sim_core(th, E)
        assert np.array_equal(pred0[0], pred1[0]) and np.array_equal(pred0[1], pred1[1]) and np.array_equal(sim0, sim1)
        after = fit.neg2loglik_grad_core(th)                 # (the prediction regrew the rows under the matrix)
        assert after[0] == first[0] and all(np.array_equal(a, b) for a, b in zip(after[1:], first[1:]))
    finally:
        fit.close()


def test_dense_and_sharded_handles_refused():
    import cocons_amd as ca
    from cocons_amd import workloads as wl, _lib
    from cocons_amd.host import _p, theta_table
    n = 200
    locs, X, th, z, _ = _setup(n, 1)
    T, mean = theta_table(th), np.ascontiguousarray(th["mean"])
    val, parts, gt, gq, gm = ctypes.c_double(0), np.zeros(2), np.zeros(18), np.zeros(18), np.zeros(3)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        L = fit._L
        rc = L.cocons_neg2loglik_grad_taper(fit._h, _p(T), _p(mean), ctypes.byref(val), _p(parts), _p(gt), _p(gq), _p(gm))
        assert rc == -1 and _lib.last_error().startswith("cocons_neg2loglik_grad_taper")
        rc = L.cocons_debug_taper_selinv(fit._h, _p(T), _p(gt), None)
        assert rc == -1 and _lib.last_error().startswith("cocons_debug_taper_selinv")
        noop_b = _lib.BCAST_FN(lambda *a: 0)
        noop_r = _lib.ALLREDUCE_FN(lambda *a: 0)
        assert L.cocons_fit_set_collectives(fit._h, 0, 2, ctypes.cast(noop_b, ctypes.c_void_p),
                                            ctypes.cast(noop_r, ctypes.c_void_p), None) == 0
        rc = L.cocons_neg2loglik_grad_taper(fit._h, _p(T), _p(mean), ctypes.byref(val), _p(parts), _p(gt), _p(gq), _p(gm))
        assert rc == -1 and _lib.last_error().startswith("cocons_neg2loglik_grad_taper")
    finally:
        fit.close()


@pytest.mark.parametrize("profile", [False, True])
def test_host_entries_with_penalty_and_safe_paths(profile):
    """GetNeg2loglikelihoodTaper_grad / ...TaperProfile_grad with a non-zero penalty: the value is the value function's, the
    gradient over the optimiser's vector agrees with Richardson central differences of the value function to 1e-6 of its
    largest component; a failing Cholesky gives (1e6, zeros) under `safe` and RuntimeError otherwise."""
    from cocons_amd import host, workloads as wl
    n, r = 700, 2
    locs, X, th, z, _ = _setup(n, r, seed=55)
    th["mean"] = np.zeros(3)
    ref_taper = _taper_pattern(locs, 0.25)
    pp = wl.par_pos_full()
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.05, 0.02, 0.3)
    fval = host.GetNeg2loglikelihoodTaperProfile if profile else host.GetNeg2loglikelihoodTaper
    fgrad = host.GetNeg2loglikelihoodTaperProfile_grad if profile else host.GetNeg2loglikelihoodTaper_grad
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        def val(x):
            return fval(x, pp, ref_taper, locs, X, wl.SMOOTH_LIMITS, z, n, lam, safe=False, fit=fit)

        v, g = fgrad(x0, pp, ref_taper, locs, X, wl.SMOOTH_LIMITS, z, n, lam, safe=False, fit=fit)
        assert abs(v - val(x0)) <= 1e-12 * abs(v)
        h = 1e-3
        num = np.zeros_like(x0)
        for i in range(x0.size):
            def d(step):
                xp, xm = x0.copy(), x0.copy()
                xp[i] += step
                xm[i] -= step
                return (val(xp) - val(xm)) / (2 * step)
            num[i] = (4 * d(h / 2) - d(h)) / 3
        print("profile=%s: %.3e of %.3e" % (profile, _inf(g - num), _inf(num)))
        assert g.shape == x0.shape
        assert _inf(g - num) <= 1e-6 * _inf(num), (g, num)
        xb = x0.copy()
        xb[0] = np.nan                                      # (a NaN parameter poisons S: the factorisation fails)
        vb, gb = fgrad(xb, pp, ref_taper, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)
        assert vb == 1e6 and gb.shape == xb.shape and np.all(gb == 0)
        with pytest.raises(RuntimeError, match="Cholesky error"):
            fgrad(xb, pp, ref_taper, locs, X, wl.SMOOTH_LIMITS, z, n, lam, safe=False, fit=fit)
    finally:
        fit.close()


def test_glue_taper_grad_matches_grad_core():
    """`_cocons_hip_neg2loglik_taper_grad` through the R stub: bit for bit what neg2loglik_grad_core returns, and a failing
    minor as a positive status with zero tables."""
    from cocons_amd import workloads as wl
    from test_glue_exec import RStub
    R = RStub()
    n, r = 700, 2
    locs, X, th, z, _ = _setup(n, r, seed=7200)
    ci, rp, ent = _taper_pattern(locs, 0.25)
    fit = _taper_fit(locs, X, z, (ci, rp, ent))
    try:
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(th)
    finally:
        fit.close()
    h = R.call("_cocons_hip_fit_create_taper", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer(ci), R.integer(rp), R.real(ent))
    st, res = R.value(R.call("_cocons_hip_neg2loglik_taper_grad", h, R.theta(th), R.real(th["mean"])))
    assert int(st[0]) == 0
    assert res[0][0] == v and np.array_equal(res[0][1:], parts)
    assert np.array_equal(res[1], gt) and np.array_equal(res[2], gq) and np.array_equal(res[3], gm)
    th_bad = {k: np.array(v_, dtype=float).copy() for k, v_ in th.items()}
    th_bad["std.dev"][0] = -np.inf
    th_bad["nugget"][0] = -np.inf
    st, res = R.value(R.call("_cocons_hip_neg2loglik_taper_grad", h, R.theta(th_bad), R.real(th["mean"])))
    assert int(st[0]) > 0 and np.all(res[1] == 0) and np.all(res[2] == 0) and np.all(res[3] == 0)
    R.L.stub_gc(0, None)
