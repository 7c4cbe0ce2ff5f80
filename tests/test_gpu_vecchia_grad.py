"""cocons_neg2loglik_grad_vecchia on the GPU against tests/vecchia_grad_reference.py, on the problems of
test_gpu_vecchia (test_gpu_dense_sizes.problem: uniform sites in no spatial order, two realisations, p = 3 from n = 3 on).

Bounds, the project's own for gradients: value and parts equal to cocons_neg2loglik_vecchia's TO THE BIT; the tables and the
mean gradient within GRAD_TOL = 1e-7 of the numpy statement, relative to the largest magnitude of the reference array; FD_TOL =
1e-6 against a Richardson difference of the device's own value entry, relative to the largest difference.  Every comparison
prints its worst error on a line that starts with `vecchia-grad-report`; the measured figures stand in
tests/golden/VECCHIA_GRAD_REPORT.md."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference as GR  # noqa: E402
import vecchia_grad_reference as VG  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402
from test_gpu_vecchia import SIZES, MS, table, pred_problem, _theta  # noqa: E402

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-7
FD_TOL = 1e-6


def _report(what, case, err):
    print("vecchia-grad-report gpu | %s | %s | %.2e" % (what, case, err))


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _limits(sl=None):
    from cocons_amd import workloads as wl
    return tuple(wl.SMOOTH_LIMITS) if sl is None else tuple(sl)


def _make(locs, X, z, nn, sl=None):
    import cocons_amd as ca
    return ca.CoconsVecchiaFit(locs, X, z, _limits(sl), nn)


def _statement(th, locs, X, z, nn, sl=None, B=None):
    from cocons_amd import host
    return VG.neg2loglik_grad(host.theta_table(th), th["mean"], locs, X, z, _limits(sl), nn, B=B)


@functools.lru_cache(maxsize=None)
def reference(n, m, holes=False):
    locs, X, th, z = problem(n)[:4]
    out = _statement(th, locs, X, z, table(n, m, holes))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _check(f, th, ref, case, B=None):
    """value bits against the value entry (B is None), the three gradients against the statement; returns the device's"""
    got = f.neg2loglik_grad_core(th, B=B)
    if B is None:
        v0, p0 = f.neg2loglik_core(th)
        assert got[0] == v0 and np.array_equal(got[1], p0), (case, got[0], v0)
    else:
        Y, logd = f.whiten_core(th, B)
        assert abs(got[1][0] - np.sum(logd)) <= 1e-12 * max(abs(np.sum(logd)), 1.0)
        assert _rel(got[1][1:], np.sum(Y * Y, axis=0)) <= 1e-12
    errs = [abs(got[0] - ref[0]) / abs(ref[0]), _rel(got[2], ref[2]),
            float(np.max(np.abs(got[3] - ref[3])) / np.max(np.abs(ref[2])))]
    if B is None:
        errs.append(_rel(got[4], ref[4]))
    _report("value table quad" + (" mean" if B is None else ""), case, max(errs))
    assert errs[0] < 1e-8 and max(errs[1:]) < GRAD_TOL, (case, errs)
    return got


def _richardson(fun, x, h=1e-4):
    g = np.zeros_like(x)
    for i in range(x.size):
        def d(step):
            xp, xm = x.copy(), x.copy()
            xp[i] += step
            xm[i] -= step
            return (fun(xp) - fun(xm)) / (2 * step)
        g[i] = (4 * d(h / 2) - d(h)) / 3
    return g


def _differences(f, th, skip_smooth=False):
    """Richardson differences of the device's own value entry over the table's entries and the mean: (table, mean)"""
    from cocons_amd import host
    keys = [k for k in host.COV_ASPECTS if not (skip_smooth and k == "smooth")]
    p = th["mean"].size
    x0 = np.concatenate([th[k] for k in keys] + [th["mean"]])

    def fun(x):
        t = OrderedDict((k, np.array(v, copy=True)) for k, v in th.items())
        for i, k in enumerate(keys):
            t[k] = x[i * p:(i + 1) * p].copy()
        t["mean"] = x[len(keys) * p:].copy()
        return f.neg2loglik_core(t)[0]

    num = _richardson(fun, x0)
    tab = np.zeros((6, p))
    for i, k in enumerate(keys):
        tab[list(host.COV_ASPECTS).index(k)] = num[i * p:(i + 1) * p]
    return tab, num[len(keys) * p:]


def _check_differences(f, th, got, case, skip_smooth=False):
    tab, gm = _differences(f, th, skip_smooth)
    scale = max(np.max(np.abs(tab)), np.max(np.abs(gm)))
    err = max(np.max(np.abs(got[2] - tab)), np.max(np.abs(got[4] - gm))) / scale
    _report("against differences of the value entry", case, err)
    assert err < FD_TOL, (case, err)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n, m):
    """rows with fewer than m predecessors, a full 64-row block (m = 63), the 64 / 65 seam, pair walks of one pass and of many"""
    locs, X, th, z = problem(n)[:4]
    f = _make(locs, X, z, table(n, m))
    try:
        _check(f, th, reference(n, m), "n%d m%d" % (n, m))
    finally:
        f.close()


@pytest.mark.parametrize("r,p", ((1, 3), (3, 3), (1, 1), (3, 1)))
def test_realisations_and_design_widths(r, p):
    n, m = 65, 10
    locs, X, th0, z = problem(n)[:4]
    z = np.asfortranarray(np.column_stack([z, np.random.default_rng(3).standard_normal(n)])[:, :r])
    X = np.asfortranarray(X[:, :p])
    th = OrderedDict((k, np.array(v[:p], copy=True)) for k, v in th0.items())
    f = _make(locs, X, z, table(n, m))
    try:
        got = _check(f, th, _statement(th, locs, X, z, table(n, m)), "n%d m%d r%d p%d" % (n, m, r, p))
        _check_differences(f, th, got, "n%d m%d r%d p%d" % (n, m, r, p))
    finally:
        f.close()


@pytest.mark.parametrize("n,m", ((65, 10), (300, 30)))
def test_tables_with_holes_and_unsorted_rows(n, m):
    locs, X, th, z = problem(n)[:4]
    nn = np.array(table(n, m, True), order="F")
    rng = np.random.default_rng(n)
    for i in range(n):
        nn[i] = nn[i, rng.permutation(m)]              # zeros anywhere, the neighbours in no order
    assert np.any(np.diff(nn[n - 1][nn[n - 1] > 0]) < 0) and np.all(nn[n // 2] == 0)
    f = _make(locs, X, z, nn)
    try:
        _check(f, th, reference(n, m, True), "holes, unsorted n%d m%d" % (n, m))
    finally:
        f.close()


@pytest.mark.parametrize("nu,slopes", ((0.5, False), (1.5, False), (2.5, False), (1.0, True)))
def test_closed_forms_and_the_bessel_branch_at_a_fixed_smoothness(nu, slopes):
    """smooth.limits equal: with a zero smooth vector the three closed forms; with slopes in it the Bessel branch at a
    smoothness that is the same everywhere (no smooth row).  The free smoothness is every other test here."""
    n, m = 300, 30
    locs, X, th0, z = problem(n)[:4]
    th = _theta(th0) if slopes else _theta(th0, smooth=np.zeros(3))
    from cocons_amd import host
    want = "geom" if slopes else {0.5: "half", 1.5: "threehalf", 2.5: "fivehalf"}[nu]
    assert GR.select_mode(host.theta_table(th), (nu, nu))[0] == want
    f = _make(locs, X, z, table(n, m), (nu, nu))
    try:
        case = "nu%.1f%s n%d m%d" % (nu, " bessel" if slopes else "", n, m)
        got = _check(f, th, _statement(th, locs, X, z, table(n, m), (nu, nu)), case)
        assert np.all(got[2][4] == 0.0) and np.all(got[3][4] == 0.0)
        _check_differences(f, th, got, case, skip_smooth=True)
    finally:
        f.close()


def test_free_smoothness_against_differences():
    n, m = 300, 30
    locs, X, th, z = problem(n)[:4]
    f = _make(locs, X, z, table(n, m))
    try:
        got = f.neg2loglik_grad_core(th)
        assert np.any(got[2][4] != 0.0)
        _check_differences(f, th, got, "free smoothness n%d m%d" % (n, m))
    finally:
        f.close()


def test_exact_with_all_predecessors():
    """n = 64, m = 63, every predecessor: the dense gradient of the numpy statement of the dense likelihood"""
    from cocons_amd import host, workloads as wl
    rng = np.random.default_rng(6464)
    n = 64
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = np.array([0.3, -0.15, 0.2])
    z = np.asfortranarray(rng.standard_normal((n, 2)))
    fv, gt, gm = GR.neg2loglik_grad(host.theta_table(th), th["mean"], locs, X, z, wl.SMOOTH_LIMITS)
    f = _make(locs, X, z, VR.all_predecessors(n))
    try:
        got = f.neg2loglik_grad_core(th)
    finally:
        f.close()
    errs = (abs(got[0] - fv) / abs(fv), _rel(got[2], gt), _rel(got[4], gm))
    _report("exact: the dense gradient", "n64 m63", max(errs))
    assert errs[0] < 1e-8 and max(errs[1:]) < GRAD_TOL, errs


def _coincident():
    """n = 65 with observation 58 (1-based) on the coordinates of observation 41, among its neighbours, with covariates that
    give it the larger variance: its block is positive definite and holds a pair with u <= eps"""
    from cocons_amd import host
    locs, X, th0, z = problem(65)[:4]
    locs, X = np.array(locs), np.array(X, order="F")
    locs[57] = locs[40]
    slope = np.array([0.0, 0.3, -0.2])
    th = _theta(th0, std_dev=slope if float((X[57] - X[40]) @ slope) > 0 else -slope)
    nn = host.vecchia_neighbours(locs, 10).copy(order="F")
    assert 41 in nn[57]
    return locs, X, th, z, nn


def test_a_coincident_pair_of_sites():
    locs, X, th, z, nn = _coincident()
    f = _make(locs, X, z, nn)
    try:
        got = _check(f, th, _statement(th, locs, X, z, nn), "coincident pair n65 m10")
        _check_differences(f, th, got, "coincident pair n65 m10")
    finally:
        f.close()


def test_a_far_pair():
    """one site 70 units away from its neighbours at a range of 0.2: u >= 706, the entry and its partials are zero"""
    from cocons_amd import host, workloads as wl
    from oracle import oracle as O
    n, m = 65, 10
    locs, X, th, z = problem(n)[:4]
    locs = np.array(locs)
    locs[50] = (50.0, 50.0)
    nn = host.vecchia_neighbours(locs, m)
    S = O.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
    assert np.all(np.abs(S[50, nn[50] - 1]) < 1e-250) and np.all(nn[50] > 0)
    f = _make(locs, X, z, nn)
    try:
        _check(f, th, _statement(th, locs, X, z, nn), "far pair n65 m10")
    finally:
        f.close()


@pytest.mark.parametrize("c", (1, 5))
def test_callers_columns(c):
    """B given: c = 1, and c = 5 -- more than one group of the forward substitution"""
    n, m = 300, 30
    locs, X, th, z = problem(n)[:4]
    B = np.asfortranarray(np.random.default_rng(c).standard_normal((n, c)))
    f = _make(locs, X, z, table(n, m))
    try:
        got = _check(f, th, _statement(th, locs, X, z, table(n, m), B=B), "B c%d n%d m%d" % (c, n, m), B=B)
        assert got[1].size == 1 + c and got[4] is None
        assert got[0] == float(sum(n * np.log(2 * np.pi) + 2 * got[1][0] + got[1][1 + k] for k in range(c)))
    finally:
        f.close()


def test_profile_and_reml_host_forms():
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    n, m = 300, 30
    locs, X, th, z = problem(n)[:4]
    pp = OrderedDict((k, [k != "mean"] * 3) for k in host.ASPECTS)
    tv = wl.theta_vector_from_lists(th, pp)
    tl = ca.getModelLists(tv, pp, "diff")
    T = host.theta_table(tl)
    lam = (0.0, 0.0, 0.0)
    nn = table(n, m)

    def vec(gt):
        g = OrderedDict(mean=np.zeros(3))
        for t, k in enumerate(host.COV_ASPECTS):
            g[k] = gt[t]
        return host.getModelLists_grad(g, pp)

    f = _make(locs, X, z, nn)
    try:
        gp = ca.GetNeg2loglikelihoodVecchiaProfile_grad(tv, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=f)
        gr = ca.GetNeg2loglikelihoodVecchiaREML_grad(tv, pp, nn, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f)
        vp = ca.GetNeg2loglikelihoodVecchiaProfile(tv, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=f)
        vr = ca.GetNeg2loglikelihoodVecchiaREML(tv, pp, nn, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f)
        pf = OrderedDict((k, [True] * 3) for k in host.ASPECTS)
        tvf = wl.theta_vector_from_lists(th, pf)
        gv = ca.GetNeg2loglikelihoodVecchia_grad(tvf, pf, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f)
        vv = ca.GetNeg2loglikelihoodVecchia(tvf, pf, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f)
        with pytest.raises(ValueError, match="rank 2 < 3"):
            Xd = np.array(X, order="F")
            Xd[:, 2] = Xd[:, 1]
            ca.GetNeg2loglikelihoodVecchiaREML_grad(tv, pp, nn, locs, Xd, Xd, wl.SMOOTH_LIMITS, z, n, lam, fit=f)
    finally:
        f.close()
    wp, wr = VG.profile_grad(T, locs, X, z, X, wl.SMOOTH_LIMITS, nn), VG.reml_grad(T, locs, X, z, wl.SMOOTH_LIMITS, nn)
    assert gv[0] == vv
    errs = (abs(gp[0] - vp) / abs(vp), abs(gr[0] - vr) / abs(vr), abs(gp[0] - wp[0]) / abs(wp[0]), abs(gr[0] - wr[0]) / abs(wr[0]))
    gerrs = (_rel(gp[1], vec(wp[1])), _rel(gr[1], vec(wr[1])))
    tlf = ca.getModelLists(tvf, pf, "diff")
    ref = _statement(tlf, locs, X, z, nn)
    g = OrderedDict(mean=ref[4])
    for t, k in enumerate(host.COV_ASPECTS):
        g[k] = ref[2][t]
    gerrs += (_rel(gv[1], host.getModelLists_grad(g, pf)),)
    _report("profile reml plain (host forms): values", "n%d m%d q3" % (n, m), max(errs))
    _report("profile reml plain (host forms): gradients", "n%d m%d q3" % (n, m), max(gerrs))
    assert max(errs) < 1e-8 and max(gerrs) < GRAD_TOL, (errs, gerrs)


def test_more_rows_than_one_chunk():
    """n above the rows of one gradient launch: a closed form and three predecessors keep it cheap.  Value bits against the
    value entry, the gradient against differences of it (no n x n reference at this size)."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 33000
    rng = np.random.default_rng(33)
    locs = np.column_stack([np.sort(rng.uniform(0, 40, size=n)), rng.uniform(0, 0.2, size=n)])      # neighbours in x
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    z = rng.standard_normal((n, 1))
    nn = np.zeros((n, 3), dtype=np.int32, order="F")
    for j in range(3):
        nn[j + 1:, j] = np.arange(1, n - j)            # row i names i - 1, i - 2, i - 3 (1-based: i, i - 1, i - 2)
    th = _theta(wl.theta_full(scale0=np.log(0.2)), smooth=np.zeros(3), mean=[0.3, -0.15, 0.2])
    f = ca.CoconsVecchiaFit(locs, X, z, (1.5, 1.5), nn)
    try:
        v0, p0 = f.neg2loglik_core(th)
        got = f.neg2loglik_grad_core(th)
        again = f.neg2loglik_grad_core(th)
        assert got[0] == v0 and np.array_equal(got[1], p0)
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], again[1:]))
        _check_differences(f, th, got, "n%d m3 nu1.5 (two chunks)" % n, skip_smooth=True)
    finally:
        f.close()


def _grad_outputs(n, m, sort):
    locs, X, th, z = problem(n)[:4]
    old = os.environ.get("COCONS_SPATIAL_SORT")
    os.environ["COCONS_SPATIAL_SORT"] = sort
    try:
        f = _make(locs, X, z, table(n, m))
        try:
            out = f.neg2loglik_grad_core(th)
        finally:
            f.close()
    finally:
        if old is None:
            os.environ.pop("COCONS_SPATIAL_SORT", None)
        else:
            os.environ["COCONS_SPATIAL_SORT"] = old
    return np.concatenate([[out[0]], out[1], out[2].ravel(), out[3].ravel(), out[4]])


@pytest.mark.parametrize("n", (65, 641))
def test_bits_repeat_and_do_not_see_the_spatial_sort(n):
    a, b, c = _grad_outputs(n, 30, "1"), _grad_outputs(n, 30, "1"), _grad_outputs(n, 30, "0")
    _report("bits: repeat, sort off", "n%d m30" % n, float(np.max(np.abs(a - c))))
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_bits_do_not_see_foreign_rows():
    """50 rows appended that name no neighbour and carry zero columns: their quadratic forms' weights are exactly zero, so
    the quadratic forms' table keeps its bits (a sum that ran over other rows' data, or in another order, would not)"""
    n, m, extra = 300, 30, 50
    locs, X, th, z = problem(n)[:4]
    rng = np.random.default_rng(9)
    B = np.asfortranarray(rng.standard_normal((n, 2)))
    locs2 = np.vstack([locs, rng.uniform(0, 1, size=(extra, 2))])
    X2 = np.asfortranarray(np.vstack([X, np.column_stack([np.ones(extra), rng.standard_normal((extra, 2))])]))
    nn2 = np.zeros((n + extra, m), dtype=np.int32, order="F")
    nn2[:n] = table(n, m)
    B2 = np.asfortranarray(np.vstack([B, np.zeros((extra, 2))]))
    f, g = _make(locs, X, z, table(n, m)), _make(locs2, X2, np.zeros((n + extra, 2)), nn2)
    try:
        a, b = f.neg2loglik_grad_core(th, B=B), g.neg2loglik_grad_core(th, B=B2)
    finally:
        f.close()
        g.close()
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[1][1:], b[1][1:])
    assert not np.array_equal(a[2], b[2])              # (the log-determinant's share does see the 50 rows)


def test_sequences_on_one_handle():
    """gradient, value, whiten and predict in both orders: every output has the bits a fresh handle gives"""
    n, m = 300, 30
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    nnp = pred_problem(n, m)[1]
    B5 = np.asfortranarray(np.random.default_rng(5).standard_normal((n, 5)))
    calls = OrderedDict(
        grad=lambda f: f.neg2loglik_grad_core(th), gradB=lambda f: f.neg2loglik_grad_core(th, B=B5)[:4],
        value=lambda f: f.neg2loglik_core(th), whiten=lambda f: f.whiten_core(th, Rz),
        predict=lambda f: f.predict_core(th, lp, Xp, nnp))

    def flat(out):
        return np.concatenate([np.ravel(np.asarray(a, dtype=float)) for a in out])

    fresh = {}
    for k, call in calls.items():
        f = _make(locs, X, z, table(n, m))
        try:
            fresh[k] = flat(call(f))
        finally:
            f.close()
    for order in (list(calls), list(calls)[::-1]):
        f = _make(locs, X, z, table(n, m))
        try:
            for k in order + order:
                assert np.array_equal(flat(calls[k](f)), fresh[k]), (order, k)
        finally:
            f.close()


def _raw(f, th, B=None):
    from cocons_amd import host
    p = f.p
    val, parts = ctypes.c_double(123.0), np.full(8, 7.0)
    gt, gq, gm = np.full(6 * p, 7.0), np.full(6 * p, 7.0), np.full(p, 7.0)
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    if B is None:
        rc = f._L.cocons_neg2loglik_grad_vecchia(f._h, host._p(T), host._p(mean), 0, None, ctypes.byref(val), host._p(parts),
                                                 host._p(gt), host._p(gq), host._p(gm))
    else:
        rc = f._L.cocons_neg2loglik_grad_vecchia(f._h, host._p(T), None, B.shape[1], host._p(B), ctypes.byref(val),
                                                 host._p(parts), host._p(gt), host._p(gq), None)
    return rc, val.value, parts, gt, gq, gm


def test_a_failing_block_is_reported_and_the_outputs_left_alone():
    """the coincident pair with the slopes of std.dev turned round: the later site has the smaller variance, the block of
    row 58 is not positive definite.  The row is returned, no output is touched, and the good theta keeps its bits."""
    locs, X, th, z, nn = _coincident()
    bad = _theta(th, std_dev=-th["std.dev"])
    f = _make(locs, X, z, nn)
    try:
        good = f.neg2loglik_grad_core(th)
        rc, val, parts, gt, gq, gm = _raw(f, bad)
        assert rc == 58 and val == 123.0 and all(np.all(a == 7.0) for a in (parts, gt, gq, gm))
        rc, val, parts, gt, gq, gm = _raw(f, bad, B=np.asfortranarray(z))
        assert rc == 58 and val == 123.0 and all(np.all(a == 7.0) for a in (parts, gt, gq))
        after = f.neg2loglik_grad_core(th)
        assert good[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(good[1:], after[1:]))
    finally:
        f.close()


def test_refusals_carry_messages():
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    n = 65
    locs, X, th, z = problem(n)[:4]
    B = np.asfortranarray(z)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    vec = _make(locs, X, z, table(n, 10))
    try:
        rc, val, parts, gt, gq, gm = _raw(dense, th)
        assert rc < 0 and val == 123.0 and np.all(gt == 7.0)
        assert _lib.last_error() == "cocons_neg2loglik_grad_vecchia: not a Vecchia fit (cocons_fit_create_vecchia makes one)"
        from cocons_amd import host
        T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
        v = ctypes.c_double(123.0)
        L = vec._L
        assert L.cocons_neg2loglik_grad_vecchia(vec._h, host._p(T), host._p(mean), 2, host._p(B), ctypes.byref(v), None,
                                                host._p(gt), None, None) < 0
        assert _lib.last_error().startswith("cocons_neg2loglik_grad_vecchia: B is given, so mean and grad_mean must be NULL")
        assert L.cocons_neg2loglik_grad_vecchia(vec._h, host._p(T), None, 0, host._p(B), ctypes.byref(v), None,
                                                host._p(gt), None, None) < 0
        assert _lib.last_error().startswith("cocons_neg2loglik_grad_vecchia: c = 0")
        assert v.value == 123.0 and np.all(gt == 7.0)
        # the dense gradient entry keeps refusing a Vecchia handle
        assert L.cocons_neg2loglik_grad_dense(vec._h, host._p(T), host._p(mean), ctypes.byref(v), None, host._p(gt),
                                              host._p(gm)) < 0
        assert _lib.last_error().startswith("cocons_neg2loglik_grad_dense: not available on a Vecchia fit")
        vec.neg2loglik_grad_core(th)                    # (the handle stays usable)
    finally:
        dense.close()
        vec.close()


def test_the_dense_gradient_keeps_its_bits_beside_vecchia_gradients():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 300
    locs, X, th, z = problem(n)[:4]
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        before = dense.neg2loglik_grad_core(th)
        f = _make(locs, X, z, table(n, 30))
        try:
            f.neg2loglik_grad_core(th)
            f.neg2loglik_grad_core(th, B=np.asfortranarray(z))
        finally:
            f.close()
        after = dense.neg2loglik_grad_core(th)
    finally:
        dense.close()
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1:], after[1:]))
