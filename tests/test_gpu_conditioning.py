"""The factorisation paths on ill-conditioned covariances (tests/conditioning_cases.py: cond(Sigma) 4e8 .. 2.5e11, against
1e2 .. 1e5 in every other parity test), judged by what each path returns against a long-double factorisation of the DEVICE'S
OWN matrix: device error <= 10 x max(LAPACK's error over six orderings, 1e-12 |reference|), quantity by quantity.  The
matrix comes from a public entry (cov_rows, cov_rns, cov_rns_pred, cov_rns_taper), so assembly error -- amplified by
cond(Sigma) like any rounding -- stays out of the comparison.  No case, ordering or schedule is skipped or excused: a "not
positive definite" from the device (CholeskyError, a non-zero return) fails the test.

Every test prints its ratios (device error / max(yardstick, floor)) on lines starting with "COND|";
tests/golden/CONDITIONING_REPORT.md holds those of one run on an MI355X."""
import contextlib
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

_DEFAULTS = (("engine", "COCONS_ENGINE", "1"), ("dag", "COCONS_DAG", "1"), ("dag_min_tiles", "COCONS_DAG_MIN_TILES", "2000"))
SCHEDULES = {
    "plain": {"engine": 0},                                   # every kernel in order on one stream
    "engine": {"engine": 1, "dag": 0},                        # diagonal tiles on the resident engine, classic updates
    "launch": {"engine": 1, "dag": 1, "dag_min_tiles": 0},    # the persistent launch for every step
}


def _tune(name, value):
    from cocons_amd import _lib
    L = _lib.load()
    _lib.check(L.cocons_debug_tune(name.encode(), int(value)), "cocons_debug_tune")


@contextlib.contextmanager
def _schedule(name):
    try:
        for k, v in SCHEDULES[name].items():
            _tune(k, v)
        yield
    finally:
        for k, env, dflt in _DEFAULTS:
            _tune(k, int(os.environ.get(env, dflt)))


def _report(path, case, n, **ratios):
    print("COND|%s|%s|%d|%s" % (path, case, n, "|".join("%s=%.3g" % kv for kv in ratios.items())))


def _check(got, yard, ref, what):
    """The measure, entry by entry; returns the largest ratio error / max(yardstick, floor)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    lim = cc.bound(yard, ref)
    assert np.all(err <= lim), "%s: ratio %.3g (error %s, bound %s)" % (what, cc.ratio(got, yard, ref), err, lim)
    return cc.ratio(got, yard, ref)


# the referee's verdict on the device's matrix of one (case, size): shared by the schedules, recomputed should an entry
# ever hand out other bits
_VERDICTS = {}


def _verdict(key, A, B):
    hit = _VERDICTS.get(key)
    if hit is None or not (np.array_equal(hit[0], A) and np.array_equal(hit[1], B)):
        hit = _VERDICTS[key] = (A.copy(), B.copy(), cc.referee(A, B))
    return hit[2]


# --------------------------------------------------------------------------- -2 loglik parts under every schedule
PARTS_CASES = [(c, gx, gy, None, False) for c, gx, gy in cc.CASE_SIZES] + \
              [(c, 28, 25, flag, shuffled) for shuffled in (False, True) for c in cc.CASES for flag in ("0", "1")]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case,gx,gy,sort,shuffled", PARTS_CASES)
def test_parts_under_every_schedule(oracle, monkeypatch, case, gx, gy, sort, shuffled, schedule):
    """sum log diag L and either realisation's quadratic form from neg2loglik_core, each by the measure, under the plain,
    the engine and the persistent-launch schedule, n = 625 / 700 / 841 (5, 6, 7 tiles); n = 700 also with the Morton sort
    off and on -- on the grid as listed (which a handle keeps in the caller's order either way: the two runs give the same
    bits) and on the same observations shuffled (sorted with the switch on; with it off the diagonal blocks hold sites from
    all over the square).  The schedule asked for really ran, no hand-off timed out, a repeat gives the same bits."""
    import cocons_amd as ca
    pb = cc.problem(case, gx, gy, shuffled)
    if sort is not None:
        monkeypatch.setenv("COCONS_SPATIAL_SORT", sort)
    with _schedule(schedule):
        fit = ca.CoconsFit(pb.locs, pb.X, pb.z, pb.smooth_limits)
        try:
            val, parts = fit.neg2loglik_core(pb.theta)
            st = fit.engine_state()
            val2, parts2 = fit.neg2loglik_core(pb.theta)
            stages = fit.profile_stages(pb.theta, reps=1)
            retries = fit.engine_state()["retries"]
            A = fit.cov_rows(pb.theta, np.arange(pb.n))
        finally:
            fit.close()
    assert retries == 0 and st["retries"] == 0
    assert val2 == val and np.array_equal(parts2, parts)
    if schedule == "plain":
        assert not st["active"] and stages["dag_ms"] == 0
    elif schedule == "engine":
        assert st["active"] and stages["dag_ms"] == 0
    else:
        assert st["active"] and stages["dag_ms"] > 0 and stages["dag_flops"] > 0
    v = _verdict((case, gx, gy, shuffled), cc.sym(A), cc.residual(pb))
    r_ld = _check(parts[0], v.yard["logdet"], v.ref["logdet"], "logdet_half")
    r_q = [_check(parts[1 + k], v.yard["quad"][k], v.ref["quad"][k], "quad[%d]" % k) for k in range(2)]
    _report("parts/%s/sort=%s%s" % (schedule, sort or "-", "s" if shuffled else ""), case, pb.n,
            logdet=r_ld, quad0=r_q[0], quad1=r_q[1], yard_logdet=v.yard["logdet"] / abs(v.ref["logdet"]),
            yard_quad0=v.yard["quad"][0] / abs(v.ref["quad"][0]), yard_quad1=v.yard["quad"][1] / abs(v.ref["quad"][1]))


# --------------------------------------------------------------------------- kriging, one-shot and held
@pytest.mark.parametrize("case", ["A", "C", "D"])
def test_kriging_one_shot_and_held(oracle, case):
    """predict_core, and krige_prepare + krige_core with max_rows 5 and 0, at 16 new sites, n = 700: stochastic and quadform
    entry by entry by the measure, reference chol_ld(A, [r, C']) finished in long double, C the device's cov_rns_pred; the
    held results do not depend on the chunking, bit for bit."""
    import cocons_amd as ca
    pb = cc.problem(case, 28, 25)
    lp, Xp = cc.pred_sites(pb)
    fit = ca.CoconsFit(pb.locs, pb.X, pb.z, pb.smooth_limits)
    try:
        got = {"one-shot": fit.predict_core(pb.theta, lp, Xp)}
        for mr in (5, 0):
            fit.krige_prepare(pb.theta, max_rows=mr)
            got["held/max_rows=%d" % mr] = fit.krige_core(lp, Xp)
        fit.krige_release()
        retries = fit.engine_state()["retries"]
        A = fit.cov_rows(pb.theta, np.arange(pb.n))
    finally:
        fit.close()
    assert retries == 0
    C = ca.cov_rns_pred(pb.theta, pb.locs, lp, pb.X, Xp, pb.smooth_limits)
    v = cc.referee_krige(cc.sym(A), cc.residual(pb)[:, 0], C)
    for path, (st, qf) in got.items():
        r_st = _check(st, v.yard["stochastic"], v.ref["stochastic"], path + " stochastic")
        r_qf = _check(qf, v.yard["quadform"], v.ref["quadform"], path + " quadform")
        _report("krige/" + path, case, pb.n, stochastic=r_st, quadform=r_qf,
                yard_stochastic=np.max(v.yard["stochastic"] / np.abs(v.ref["stochastic"])),
                yard_quadform=np.max(v.yard["quadform"] / np.abs(v.ref["quadform"])))
    for k in range(2):
        assert np.array_equal(got["held/max_rows=5"][k], got["held/max_rows=0"][k])


# --------------------------------------------------------------------------- the factor itself
def _chol_solve(A, rhs=None):
    from cocons_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    n = A.shape[0]
    A = np.asfortranarray(A)
    L = np.zeros((n, n), order="F")
    ld = ctypes.c_double()
    if rhs is None:
        rc = lib.cocons_chol_solve(n, A.ctypes.data_as(dp), 0, None, L.ctypes.data_as(dp), None, ctypes.byref(ld))
        Y = None
    else:
        rhs = np.asfortranarray(rhs)
        Y = np.zeros(rhs.shape, order="F")
        rc = lib.cocons_chol_solve(n, A.ctypes.data_as(dp), rhs.shape[1], rhs.ctypes.data_as(dp), L.ctypes.data_as(dp),
                                   Y.ctypes.data_as(dp), ctypes.byref(ld))
    assert rc == 0, (rc, _lib.last_error())
    return L, Y, ld.value


@pytest.mark.parametrize("case", cc.HARD)
def test_factor_itself_plain_schedule(oracle, case):
    """cocons_chol_solve on the device's Sigma, n = 625, three right-hand sides: logdet_half and L^-1 B (column by column,
    maximum norm) by the measure; max |L L' - A| / max |A| (product in long double) within 10 x max(LAPACK's over the six
    orderings, 1e-15).  No componentwise bound: an inverse-based solve does not satisfy that theorem."""
    import cocons_amd as ca
    pb = cc.problem(case, 25, 25)
    A = cc.sym(ca.cov_rns(pb.theta, pb.locs, pb.X, pb.smooth_limits))
    B = np.column_stack([cc.residual(pb), np.random.default_rng(11).standard_normal(pb.n)])
    L, Y, ld = _chol_solve(A, B)
    v = cc.referee_factor(A, B)
    r_ld = _check(ld, v.yard["logdet"], v.ref["logdet"], "logdet_half")
    err_Y = np.max(np.abs(Y - v.ref["Y"]), axis=0)
    max_Y = np.max(np.abs(v.ref["Y"]), axis=0)
    lim_Y = np.maximum(v.yard["Y"], cc.FLOOR * max_Y)
    r_Y = float(np.max(err_Y / lim_Y))
    assert np.all(err_Y <= cc.FACTOR * lim_Y), ("Y: ratio %.3g" % r_Y, err_Y, v.yard["Y"], max_Y)
    res = cc.product_residual(L, A)
    lim = cc.FACTOR * max(v.yard["residual"], cc.RESIDUAL_FLOOR)
    _report("chol_solve", case, pb.n, logdet=r_ld, Y=r_Y, residual=res / (lim / cc.FACTOR),
            yard_logdet=v.yard["logdet"] / abs(v.ref["logdet"]), yard_Y=np.max(v.yard["Y"] / max_Y),
            yard_residual=v.yard["residual"])
    assert res <= lim, (res, v.yard["residual"])


@pytest.mark.parametrize("k", [-400, -100, 100, 400])
def test_pivot_scaling(k):
    """rsqrt_pivot away from pivots of order 1: the matrix of test_chol_solve_vs_long_double (n = 300) times 4^k -- an exact
    scaling, nothing under- or overflows -- must give L = 2^k L(k = 0) within 2 ulp per entry and logdet_half = logdet_half(0)
    + n k ln 2 to 1e-13 relative.  (The algebra says the bits are the same; the printed line says whether they were.)"""
    n = 300
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n))
    A = G @ G.T + n * np.eye(n)
    L0, _, ld0 = _chol_solve(A)
    Lk, _, ldk = _chol_solve(np.ldexp(A, 2 * k))
    want = np.ldexp(L0, k)
    assert np.all(np.isfinite(Lk)) and np.all(np.diag(Lk) > 0)
    ulp = np.abs(Lk - want) / np.spacing(np.abs(want))
    want_ld = ld0 + n * k * math.log(2.0)
    print("COND|scaling|k=%d|max_ulp=%.3g|identical=%s|logdet_rel=%.3g"
          % (k, ulp.max(), np.array_equal(Lk, want), abs(ldk - want_ld) / abs(want_ld)))
    assert ulp.max() <= 2.0
    assert abs(ldk - want_ld) <= 1e-13 * abs(want_ld)


# --------------------------------------------------------------------------- the band-limited schedule
@pytest.mark.parametrize("case", ["A", "D"])
def test_band_limited_schedule_on_the_full_pattern(oracle, case):
    """A taper handle on the FULL pattern with all-ones taper entries, n = 700: S is the model's covariance and stays
    ill-conditioned (real Wendland tapers give cond <= 1e5 at these parameters and test nothing of this).  The full pattern is
    NOT routed away from the band-limited factorisation: the envelope of every tile column reaches the last tile row (W = nt,
    hence the unpacked buffer), and a taper handle keeps to the plain schedule (engine not active) -- both asserted.  The
    parts of the value entry by the measure against the dense matrix of the device's cov_rns_taper entries."""
    import cocons_amd as ca
    pb = cc.problem(case, 28, 25)
    n = pb.n
    ci = np.tile(np.arange(1, n + 1, dtype=np.int32), n)
    rp = 1 + n * np.arange(n + 1, dtype=np.int32)
    fit = ca.CoconsTaperFit(pb.locs, pb.X, pb.z, pb.smooth_limits, ci, rp, np.ones(ci.size))
    try:
        val, parts = fit.neg2loglik_core(pb.theta)
        st = fit.engine_state()
        val2, parts2 = fit.neg2loglik_core(pb.theta)
        fit.krige_taper_prepare(pb.theta)
        info = fit.krige_taper_info()
        fit.krige_taper_release()
    finally:
        fit.close()
    assert val2 == val and np.array_equal(parts2, parts)
    assert st["retries"] == 0 and not st["active"]
    assert info["nt"] == 6 and info["W"] == info["nt"]
    A = cc.sym(ca.cov_rns_taper(pb.theta, pb.locs, pb.X, ci, rp, pb.smooth_limits).reshape(n, n))
    v = cc.referee(A, cc.residual(pb))
    r_ld = _check(parts[0], v.yard["logdet"], v.ref["logdet"], "logdet_half")
    r_q = [_check(parts[1 + k], v.yard["quad"][k], v.ref["quad"][k], "quad[%d]" % k) for k in range(2)]
    _report("taper/full-pattern", case, n, logdet=r_ld, quad0=r_q[0], quad1=r_q[1],
            yard_logdet=v.yard["logdet"] / abs(v.ref["logdet"]), yard_quad0=v.yard["quad"][0] / abs(v.ref["quad"][0]),
            yard_quad1=v.yard["quad"][1] / abs(v.ref["quad"][1]))
