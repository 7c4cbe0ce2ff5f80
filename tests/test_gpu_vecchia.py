"""The Vecchia entries on the GPU (cocons_fit_create_vecchia, cocons_neg2loglik_vecchia, cocons_vecchia_whiten,
cocons_vecchia_predict) against tests/vecchia_reference.py on the oracle's matrices, on the problem of
test_gpu_dense_sizes.problem (uniform sites in no spatial order, p = 3, two realisations, theta_full(scale0 = log 0.2)) and one
fixed-smoothness theta per closed-form mode.

Bound of every comparison with the reference: the project's parity bound, PARITY = 1e-8 of test_gpu_dense_sizes, relative to
the largest magnitude of the compared array or to |value|.  Every test prints its worst error on one line that starts with
`vecchia-report`; the measured figures stand in tests/golden/VECCHIA_REPORT.md."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import PARITY, problem  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 65, 300, 641)
MS = (1, 10, 30, 63)


def _report(what, case, err):
    print("vecchia-report gpu | %s | %s | %.2e" % (what, case, err))


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


@functools.lru_cache(maxsize=None)
def table(n, m, holes=False):
    """the m nearest earlier observations; holes: zeros in the middle of every third row and one all-zero row"""
    from cocons_amd import host
    nn = host.vecchia_neighbours(problem(n)[0], m)
    if holes:
        nn = nn.copy(order="F")
        nn[::3, m // 2] = 0
        nn[::3, 0] = 0
        nn[n // 2, :] = 0
    nn.setflags(write=False)
    return nn


@functools.lru_cache(maxsize=None)
def reference(n, m, holes=False):
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    Y, logd = VR.whiten(S, table(n, m, holes), Rz)
    val, parts = VR.neg2loglik(S, table(n, m, holes), Rz)
    for a in (Y, logd, parts):
        a.setflags(write=False)
    return val, parts, Y, logd


def _fit(n, m, holes=False, smooth_limits=None, nn=None):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = problem(n)[:4]
    return ca.CoconsVecchiaFit(locs, X, z, smooth_limits or wl.SMOOTH_LIMITS, table(n, m, holes) if nn is None else nn)


def _check_against(f, th, Rz, ref, case):
    val, parts, Y, logd = ref
    gv, gp = f.neg2loglik_core(th)
    gY, glogd = f.whiten_core(th, Rz)
    errs = (abs(gv - val) / abs(val), _rel(gp, parts), _rel(gY, Y), _rel(glogd, logd))
    _report("value parts whitened logd", case, max(errs))
    assert max(errs) < PARITY, errs


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_value_parts_whitened_columns_and_logd(n, m):
    """rows with fewer than m predecessors, a full 64-row block (m = 63), the 64 / 65 seam, a ragged last tile (641)"""
    th, Rz = problem(n)[2], problem(n)[7]
    f = _fit(n, m)
    try:
        _check_against(f, th, Rz, reference(n, m), "n%d m%d" % (n, m))
    finally:
        f.close()


@pytest.mark.parametrize("n,m", ((65, 10), (300, 30)))
def test_tables_with_zeros_inside_rows_and_an_empty_row(n, m):
    th, Rz = problem(n)[2], problem(n)[7]
    assert np.all(table(n, m, True)[n // 2] == 0) and table(n, m, True)[30, m // 2] == 0 and table(n, m, True)[30, m - 1] > 0
    f = _fit(n, m, True)
    try:
        _check_against(f, th, Rz, reference(n, m, True), "holes n%d m%d" % (n, m))
    finally:
        f.close()


@pytest.mark.parametrize("nu", (0.5, 1.5, 2.5))
def test_closed_form_modes(nu):
    """a fixed smoothness (smooth.limits equal, a zero smooth vector): the closed forms the dense assembly would choose"""
    from oracle import oracle as O
    n, m = 300, 30
    locs, X, th0, z = problem(n)[:4]
    th = OrderedDict((k, np.array(v, copy=True)) for k, v in th0.items())
    th["smooth"] = np.zeros(3)
    S = O.cov_rns(th, locs, X, (nu, nu))
    Rz = z - (X @ th["mean"])[:, None]
    val, parts = VR.neg2loglik(S, table(n, m), Rz)
    Y, logd = VR.whiten(S, table(n, m), Rz)
    f = _fit(n, m, smooth_limits=(nu, nu))
    try:
        _check_against(f, th, Rz, (val, parts, Y, logd), "nu%.1f n%d m%d" % (nu, n, m))
    finally:
        f.close()


def test_exact_with_all_predecessors():
    """n = 64, m = 63, every predecessor: the dense value, by the dense handle and by numpy"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    rng = np.random.default_rng(6464)
    n = 64
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = np.array([0.3, -0.15, 0.2])
    z = rng.standard_normal((n, 2))
    S = O.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
    exact = VR.neg2loglik_exact(S, z - (X @ th["mean"])[:, None])
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    d = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        got, dense = f.neg2loglik_core(th)[0], d.neg2loglik_core(th)[0]
    finally:
        f.close()
        d.close()
    errs = (abs(got - dense) / abs(dense), abs(got - exact) / abs(exact))
    _report("exact, dense handle and numpy", "n64 m63", max(errs))
    assert max(errs) < PARITY, errs


def test_profile_and_reml_host_forms():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    n, m = 300, 30
    locs, X, th, z = problem(n)[:4]
    pp = wl.par_pos_full()
    tv = wl.theta_vector_from_lists(th, pp)
    tl = ca.getModelLists(tv, pp, "diff")
    S = O.cov_rns(tl, locs, X, wl.SMOOTH_LIMITS)
    lam = (0.0, 0.0, 0.0)
    f = _fit(n, m)
    try:
        gp = ca.GetNeg2loglikelihoodVecchiaProfile(tv, pp, table(n, m), locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=f)
        gr = ca.GetNeg2loglikelihoodVecchiaREML(tv, pp, table(n, m), locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f)
        gv = ca.GetNeg2loglikelihoodVecchia(tv, pp, table(n, m), locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f)
    finally:
        f.close()
    wp, wr = VR.profile_value(S, table(n, m), z, X), VR.reml_value(S, table(n, m), z, X)
    wv = VR.neg2loglik(S, table(n, m), z - (X @ tl["mean"])[:, None])[0]
    errs = (abs(gp - wp) / abs(wp), abs(gr - wr) / abs(wr), abs(gv - wv) / abs(wv))
    _report("profile reml value (host forms)", "n%d m%d q3" % (n, m), max(errs))
    assert max(errs) < PARITY, errs


@functools.lru_cache(maxsize=None)
def pred_problem(n, m_pred):
    """70 rows: row 3 sits exactly on observation 17, which is among its neighbours; row 5 has no neighbours"""
    from cocons_amd import host, workloads as wl
    from oracle import oracle as O
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    lp = np.array(lp)
    lp[3] = locs[17]
    nnp = host.vecchia_neighbours_pred(locs, lp, m_pred).copy(order="F")
    assert 18 in nnp[3]
    nnp[5, :] = 0
    C = O.cov_rns_pred(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS)
    st, qf = VR.predict(S, C, nnp, Rz[:, 1])
    for a in (lp, nnp, st, qf):
        a.setflags(write=False)
    return lp, nnp, st, qf


@pytest.mark.parametrize("m_pred", (1, 30, 63))
@pytest.mark.parametrize("n", (300, 641))
def test_prediction(n, m_pred):
    th, Xp = problem(n)[2], problem(n)[5]
    lp, nnp, st, qf = pred_problem(n, m_pred)
    f = _fit(n, 10)
    try:
        gs, gq = f.predict_core(th, lp, Xp, nnp, z_col=1)
        hs = [f.predict_core(th, lp[a:b], Xp[a:b], nnp[a:b], z_col=1) for a, b in ((0, 35), (35, 70))]
        # more rows than one chunk holds: the 70 rows over and over; every copy gives the bits of the first
        reps = f.info()["rows"] // 70 + 2
        ts, tq = f.predict_core(th, np.tile(lp, (reps, 1)), np.tile(Xp, (reps, 1)), np.tile(nnp, (reps, 1)), z_col=1)
    finally:
        f.close()
    errs = (_rel(gs, st), _rel(gq, qf))
    _report("prediction stochastic quadform", "n%d m_pred%d" % (n, m_pred), max(errs))
    assert max(errs) < PARITY, errs
    assert gs[5] == 0.0 and gq[5] == 0.0
    assert np.array_equal(np.concatenate([h[0] for h in hs]), gs) and np.array_equal(np.concatenate([h[1] for h in hs]), gq)
    assert np.array_equal(ts, np.tile(gs, reps)) and np.array_equal(tq, np.tile(gq, reps))


def _all_outputs(n, m):
    th, Xp, Rz = problem(n)[2], problem(n)[5], problem(n)[7]
    lp, nnp = pred_problem(n, m)[:2]
    f = _fit(n, m)
    try:
        v, parts = f.neg2loglik_core(th)
        Y, logd = f.whiten_core(th, Rz)
        st, qf = f.predict_core(th, lp, Xp, nnp)
    finally:
        f.close()
    return np.concatenate([[v], parts, Y.ravel(), logd, st, qf])


@pytest.mark.parametrize("n", (65, 641))
def test_bits_repeat_and_do_not_see_the_spatial_sort(n):
    old = os.environ.get("COCONS_SPATIAL_SORT")
    try:
        os.environ["COCONS_SPATIAL_SORT"] = "1"
        a, b = _all_outputs(n, 30), _all_outputs(n, 30)
        os.environ["COCONS_SPATIAL_SORT"] = "0"
        c = _all_outputs(n, 30)
    finally:
        if old is None:
            os.environ.pop("COCONS_SPATIAL_SORT", None)
        else:
            os.environ["COCONS_SPATIAL_SORT"] = old
    _report("bits: repeat, sort off", "n%d m30" % n, float(np.max(np.abs(a - c))))
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_a_row_does_not_see_the_other_rows_lists():
    n, m = 300, 30
    th, Rz = problem(n)[2], problem(n)[7]
    nn = table(n, m).copy(order="F")
    keep = np.arange(n) % 2 == 0
    nn[~keep, 1:] = 0                       # every odd row keeps its nearest neighbour only
    f, g = _fit(n, m), _fit(n, m, nn=nn)
    try:
        (Y0, l0), (Y1, l1) = f.whiten_core(th, Rz), g.whiten_core(th, Rz)
    finally:
        f.close()
        g.close()
    assert not np.array_equal(Y0[~keep], Y1[~keep])
    assert np.array_equal(Y0[keep], Y1[keep]) and np.array_equal(l0[keep], l1[keep])


def _duplicate_site(same_covariates):
    """n = 65 with observation 58 (1-based) on the coordinates of observation 41 and conditioned on it alone"""
    from cocons_amd import host
    locs, X, th, z = problem(65)[:4]
    locs, X = np.array(locs), np.array(X, order="F")
    locs[57] = locs[40]
    if same_covariates:
        X[57] = X[40]
    nn = host.vecchia_neighbours(locs, 10).copy(order="F")
    nn[57, :] = 0
    nn[57, 0] = 41
    return locs, X, th, z, nn


def _theta(th0, **over):
    th = OrderedDict((k, np.array(v, copy=True)) for k, v in th0.items())
    th.update((k.replace("_", "."), np.asarray(v, dtype=float)) for k, v in over.items())
    return th


def _raw_value(f, th):
    from cocons_amd import host
    val, parts = ctypes.c_double(123.0), np.full(1 + f.r, 7.0)
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    rc = f._L.cocons_neg2loglik_vecchia(f._h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts))
    return rc, val.value, parts


def test_failing_block_is_reported_and_the_value_left_alone():
    """Identical coordinates AND covariates: the pair's entry is the sites' common diagonal value (the reference's u <= eps
    rule), so the block of row 58 is a [[1, 1], [1, 1]] (unit variance, no nugget: its second pivot is exactly 0) at this theta
    and singular at any other"""
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    locs, X, th0, z, nn = _duplicate_site(True)
    bad = _theta(th0, std_dev=np.zeros(3), nugget=[-np.inf, 0.0, 0.0])
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        rc, val, parts = _raw_value(f, bad)
        assert rc == 58 and val == 123.0 and np.all(parts == 7.0)
        with pytest.raises(_lib.CholeskyError) as e:
            f.whiten_core(bad, z)
        assert e.value.minor == 58
        assert _raw_value(f, bad)[0] == 58
    finally:
        f.close()
    _report("failing block", "n65 row 58", 0.0)


def test_a_good_theta_keeps_its_bits_after_failures():
    """Identical coordinates, different covariates: the block of row 58 is [[a, a], [a, b]] with a, b the two sites' variances,
    so the sign of the std.dev slopes decides whether it has a positive second pivot.  After the failing theta, and after a
    NaN theta, the good one gives the bits it gave before."""
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    locs, X, th0, z, nn = _duplicate_site(False)
    slope = np.array([0.0, 0.3, -0.2])
    up = float((X[57] - X[40]) @ slope) > 0                # b > a with these slopes
    good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
    nan = _theta(th0)
    nan["scale"][1] = np.nan
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        v0, p0 = f.neg2loglik_core(good)
        Y0, l0 = f.whiten_core(good, z)
        rc, val, parts = _raw_value(f, bad)
        assert rc == 58 and val == 123.0 and np.all(parts == 7.0)
        v1, p1 = f.neg2loglik_core(good)
        assert v1 == v0 and np.array_equal(p1, p0)
        rc, val, parts = _raw_value(f, nan)
        assert rc > 0 and val == 123.0
        with pytest.raises(_lib.CholeskyError):
            f.whiten_core(nan, z)
        v2, p2 = f.neg2loglik_core(good)
        Y2, l2 = f.whiten_core(good, z)
        assert v2 == v0 and np.array_equal(p2, p0) and np.array_equal(Y2, Y0) and np.array_equal(l2, l0)
    finally:
        f.close()


def test_refusals_carry_messages():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n = 65
    locs, X, th, z = problem(n)[:4]
    good = np.array(table(n, 10), order="F")

    def refused(nn, *words):
        with pytest.raises(_lib.CoconsHipError) as e:
            ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
        assert all(w in str(e.value) for w in ("cocons_fit_create_vecchia",) + words), str(e.value)

    refused(np.zeros((n, 0), dtype=np.int32), "m = 0")
    refused(np.zeros((n, 64), dtype=np.int32), "m = 64")
    late = good.copy(order="F")
    late[5, 0] = 6                        # row 6 names itself
    refused(late, "row 6 ")
    twice = good.copy(order="F")
    twice[10, 0] = twice[10, 1] = 3
    refused(twice, "row 11 ", "twice")
    bad_locs = np.array(locs)
    bad_locs[7, 1] = np.inf
    with pytest.raises(_lib.CoconsHipError) as e:
        ca.CoconsVecchiaFit(bad_locs, X, z, wl.SMOOTH_LIMITS, good)
    assert "cocons_fit_create_vecchia" in str(e.value) and "not finite" in str(e.value)
    # the wrong kind of handle
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    val, parts = ctypes.c_double(0.0), np.zeros(3)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    taper = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, 0.2)
    vec = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, good)
    try:
        L = vec._L
        for h in (dense, taper):
            assert L.cocons_neg2loglik_vecchia(h._h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts)) < 0
            assert _lib.last_error() == "cocons_neg2loglik_vecchia: not a Vecchia fit (cocons_fit_create_vecchia makes one)"
            out = np.zeros((n, 2), order="F")
            assert L.cocons_vecchia_whiten(h._h, host._p(T), 2, host._p(np.asfortranarray(z)), host._p(out), None) < 0
            assert _lib.last_error().startswith("cocons_vecchia_whiten: not a Vecchia fit")
        assert L.cocons_neg2loglik_dense(vec._h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts)) < 0
        assert _lib.last_error().startswith("cocons_neg2loglik_dense: not available on a Vecchia fit")
        assert L.cocons_krige_prepare(vec._h, host._p(T), host._p(mean), 0, 0) < 0 and "Vecchia" in _lib.last_error()
        lp = np.asfortranarray(problem(n)[4])
        st = np.zeros(70)
        nnp = np.full((70, 2), n + 1, dtype=np.int32, order="F")
        assert L.cocons_vecchia_predict(vec._h, host._p(T), host._p(mean), 0, 70, host._p(lp),
                                        host._p(problem(n)[5]), 2, host._ip(nnp), host._p(st), host._p(st)) < 0
        assert "row 1 of nn_pred" in _lib.last_error()
    finally:
        for h in (dense, taper, vec):
            h.close()


def test_existing_entries_keep_their_bits_beside_vecchia_calls():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 300
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        before = dense.neg2loglik_core(th)
        f = _fit(n, 30)
        try:
            f.neg2loglik_core(th)
            f.whiten_core(th, Rz)
            f.predict_core(th, lp, Xp, pred_problem(n, 30)[1])
        finally:
            f.close()
        after = dense.neg2loglik_core(th)
    finally:
        dense.close()
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
