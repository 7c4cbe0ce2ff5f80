"""The later entries of a dense fit -- Fisher information, REML information, cross-validation, held-factor kriging, joint
prediction -- below the sizes their own tests start at (130 and 300): one observation, two, the 64 / 65 seam where the
Morton sort of a handle switches on, one tile nearly full and full (127, 128: front padding 1 and 0), one observation past a
tile edge (129: front padding at its largest) and two whole tiles (256).  p = 1 below three observations (the intercept
alone), else p = 3; two realisations; 70 prediction rows (a 64-row chunk and a chunk of 6).

Each entry is held against its existing reference module at the tolerance constant of its existing test (imported; where
that test states a literal, the literal is named at the comparison).  After each entry neg2loglik_core gives the bits it gave
before, and no handle fell back from the engine schedule (engine_state()["retries"] == 0).  n = 65 and 129 also run with
COCONS_SPATIAL_SORT=0: per-observation outputs agree between sort on and sort off within the entry's tolerance, in the
caller's order.  Every test prints its worst errors in one line that starts with `sizes-report`."""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
import fisher_reference as FR  # noqa: E402
import fisher_reml_reference as RR  # noqa: E402
import krige_joint_reference as KJ  # noqa: E402
from test_gpu_cv import BOUND as CV_BOUND  # noqa: E402
from test_gpu_fisher import TOL as FISHER_TOL  # noqa: E402
from test_gpu_krige import TOL as KRIGE_TOL, _assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

DENSE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 256)
SORT_OFF_SIZES = (65, 129)
M_PRED = 70
R = 2
PARITY = 1e-8            # the literal of test_gpu_krige_joint.test_joint_against_oracle: the project's parity bound
sizes = pytest.mark.parametrize("n", DENSE_SIZES)


def _report(entry, n, text):
    print("sizes-report dense | %s | n%d | %s" % (entry, n, text))


def _inf(a):
    return float(np.max(np.abs(a)))


@functools.lru_cache(maxsize=None)
def problem(n):
    """(locs, X, theta, z, lp, Xp, Sigma, R) from fixed seeds, the oracle's Sigma; computed once, read-only.  Uniform sites
    (in no spatial order: what the Morton sort rearranges), the design of test_ragged_sizes_all_entry_points."""
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(6400 + n)
    p = 1 if n < 3 else 3
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n)] + [rng.standard_normal(n) * 0.5 for _ in range(p - 1)]))
    th = OrderedDict((k, np.array(v[:p], dtype=float)) for k, v in wl.theta_full(scale0=np.log(0.2)).items())
    th["mean"] = np.array([0.3, -0.15, 0.2])[:p]
    z = np.asfortranarray(rng.standard_normal((n, R)))
    lp = rng.uniform(0, 1, size=(M_PRED, 2))
    Xp = np.asfortranarray(np.column_stack([np.ones(M_PRED)] + [rng.standard_normal(M_PRED) * 0.5 for _ in range(p - 1)]))
    S = O.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
    Rz = z - (X @ th["mean"])[:, None]
    for a in (locs, X, z, lp, Xp, S, Rz) + tuple(th.values()):
        a.setflags(write=False)
    return locs, X, th, z, lp, Xp, S, Rz


def _units(p):
    return np.eye(6 * p).reshape(6 * p, 6, p)


@functools.lru_cache(maxsize=None)
def _ref_fisher(n):
    """(I at r = 1 by fisher_reference, I_R at r = 1 by fisher_reml_reference's projector or None at n = p, X' Sigma^-1 X on the
    oracle's Sigma) for the 6 p unit directions"""
    from cocons_amd import host, workloads as wl
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    p = X.shape[1]
    Sg, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, _units(p))
    out = (FR.info_solve(Sg, Sa, 1), RR.info_projector(Sg, Sa, X, 1) if n > p else None, X.T @ np.linalg.solve(S, X))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def _folds(n):
    """the fold layouts of a size: leave-one-out; two folds of ceil(n / 2) and floor(n / 2) (n >= 2); one fold holding all but
    one observation (n >= 3) -- at n = 129 and 256 a fold above the 128 observations a fold may have to be factored in LDS"""
    out = OrderedDict(loo=None)
    if n >= 2:
        out["two"] = np.random.default_rng(n).permutation(n) % 2
    if n >= 3:
        lab = np.zeros(n, dtype=int)
        lab[n // 2] = 1
        out["all_but_one"] = lab
    return out


@functools.lru_cache(maxsize=None)
def _ref_cv(n, layout):
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    lab = _folds(n)[layout]
    out = CV.cv_brute(S, Rz, np.arange(n) if lab is None else lab)
    for a in out:
        a.setflags(write=False)
    return out


def _fit(monkeypatch, n, sort=True):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    monkeypatch.delenv("COCONS_SPATIAL_SORT", raising=False)
    if not sort:
        monkeypatch.setenv("COCONS_SPATIAL_SORT", "0")
    locs, X, th, z = problem(n)[:4]
    return ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)


class _Unchanged:
    """neg2loglik_core before and after an entry: the same bits; no engine time-out on the handle"""

    def __init__(self, fit, th):
        self.fit, self.th = fit, th
        self.first = fit.neg2loglik_core(th)

    def check(self, what):
        again = self.fit.neg2loglik_core(self.th)
        assert again[0] == self.first[0] and np.array_equal(again[1], self.first[1]), "the value's bits after " + what
        assert self.fit.engine_state()["retries"] == 0, what


# --------------------------------------------------------------------------- entries
@sizes
def test_value_first(monkeypatch, n):
    """the value every other test here asks for again, against the long-double factorisation of the oracle's Sigma (1e-9: test_ragged_sizes_all_entry_points)"""
    from oracle import oracle as O
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    fit = _fit(monkeypatch, n)
    try:
        val, parts = fit.neg2loglik_core(th)
        assert fit.engine_state()["retries"] == 0
    finally:
        fit.close()
    info, ld, quad, _ = O.chol_ld(S, Rz)
    assert info == 0
    truth = sum(n * np.log(2 * np.pi) + 2 * ld + q for q in quad)
    _report("value", n, "value %.2e parts %.2e" % (abs(val - truth) / abs(truth), _inf(parts[1:] / quad - 1)))
    assert abs(val - truth) <= 1e-9 * abs(truth)
    assert np.allclose(parts[1:], quad, rtol=1e-9, atol=0)


@sizes
def test_fisher(monkeypatch, n):
    """fisher_core for the 6 p unit directions against tests/fisher_reference.py (FISHER_TOL in its metric:
    test_unit_directions_against_reference), info_mean against r X' Sigma^-1 X on the oracle's Sigma (1e-10: _check_mean);
    symmetric to the bit; a repeated call gives the same bits."""
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    p = X.shape[1]
    I, _, Im = _ref_fisher(n)
    fit = _fit(monkeypatch, n)
    try:
        keep = _Unchanged(fit, th)
        info, info_mean = fit.fisher_core(th, _units(p))
        keep.check("fisher_core")
        again = fit.fisher_core(th, _units(p))
    finally:
        fit.close()
    gap = FR.metric(info, R * I)
    gm = _inf(info_mean - R * Im) / _inf(R * Im)
    v_s = FR.scaling_direction(p).ravel()
    ident = float(v_s @ info @ v_s) - R * n / 2
    _report("fisher", n, "gap %.2e info_mean %.2e I(v_s, v_s) - r n / 2 %.2e" % (gap, gm, ident))
    assert info.shape == (6 * p, 6 * p) and info_mean.shape == (p, p)
    assert gap <= FISHER_TOL
    assert gm <= 1e-10
    assert abs(ident) <= 1e-9 * R * n / 2          # (test_identities' bound at its smaller size)
    assert np.array_equal(info, info.T)
    assert np.array_equal(again[0], info) and np.array_equal(again[1], info_mean)


@pytest.mark.parametrize("n", [n for n in DENSE_SIZES if n >= 2])
def test_fisher_reml(monkeypatch, n):
    """fisher_reml_core for the 6 p unit directions against the projector form of tests/fisher_reml_reference.py (FISHER_TOL:
    test_gpu_fisher_reml.test_unit_directions_against_reference); I_R(v_s, v_s) = r (n - p) / 2; symmetric to the bit.  n = 2
    with the intercept alone leaves one error contrast."""
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    p = X.shape[1]
    IR = _ref_fisher(n)[1]
    fit = _fit(monkeypatch, n)
    try:
        keep = _Unchanged(fit, th)
        info = fit.fisher_reml_core(th, _units(p))
        keep.check("fisher_reml_core")
        again = fit.fisher_reml_core(th, _units(p))
    finally:
        fit.close()
    gap = FR.metric(info, R * IR)
    v_s = FR.scaling_direction(p).ravel()
    ident = float(v_s @ info @ v_s) - R * (n - p) / 2
    _report("fisher reml", n, "gap %.2e I_R(v_s, v_s) - r (n - p) / 2 %.2e" % (gap, ident))
    assert gap <= FISHER_TOL
    assert abs(ident) <= 1e-9 * R * n / 2
    assert np.array_equal(info, info.T) and np.array_equal(again, info)


@sizes
def test_cross_validation(monkeypatch, n):
    """cv_core against cv_reference.cv_brute on the oracle's Sigma, gap_e and gap_v within CV_BOUND (test_gpu_cv.check):
    leave-one-out, two folds of ceil(n / 2) and floor(n / 2), one fold of all but one observation.  n = 1: leaving the one
    observation out leaves nothing -- the error is the residual, the variance Sigma_11.  n <= 128: a fold that is factored in
    LDS can be the whole data set but one."""
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    fit = _fit(monkeypatch, n)
    got = OrderedDict()
    try:
        keep = _Unchanged(fit, th)
        for layout, lab in _folds(n).items():
            got[layout] = fit.cv_core(th, lab)
            keep.check("cv_core " + layout)
        again = fit.cv_core(th)
    finally:
        fit.close()
    text = []
    for layout, (e, v) in got.items():
        lab = _folds(n)[layout]
        if layout == "two":
            assert sorted(np.bincount(lab).tolist()) == [n // 2, n - n // 2]
        if layout == "all_but_one":
            assert sorted(np.bincount(lab).tolist()) == [1, n - 1]
        we, wv = _ref_cv(n, layout)
        ge, gv = CV.gaps(e, v, we, wv)
        text.append("%s gap_e %.2e gap_v %.2e" % (layout, ge, gv))
        assert e.shape == (n, R) and v.shape == (n,)
    _report("cross-validation", n, "; ".join(text))
    for layout, (e, v) in got.items():
        ge, gv = CV.gaps(e, v, *_ref_cv(n, layout))
        assert ge <= CV_BOUND and gv <= CV_BOUND, (layout, ge, gv)
    if n == 1:
        we, wv = _ref_cv(1, "loo")
        assert np.array_equal(we, Rz) and wv[0] == S[0, 0]
    assert np.array_equal(again[0], got["loo"][0]) and np.array_equal(again[1], got["loo"][1])


@sizes
def test_held_factor_kriging(monkeypatch, n):
    """krige_prepare with max_rows 1, 64 and the default, then krige_core on the 70 rows: against predict_core on the same
    handle (KRIGE_TOL: test_krige_matches_predict_core); the three chunkings give the same bits."""
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    fit = _fit(monkeypatch, n)
    outs = []
    try:
        keep = _Unchanged(fit, th)
        want = fit.predict_core(th, lp, Xp)
        keep.check("predict_core")
        for max_rows in (1, 64, 0):
            fit.krige_prepare(th, max_rows=max_rows)
            info = fit.krige_info()
            # (a chunk is whole 64-row strips, one at least: max_rows = 1 is cut into the chunks of max_rows = 64)
            assert info["prepared"] and info["n"] == n and (max_rows == 0 or info["rows"] == max(max_rows // 64 * 64, 64)), info
            outs.append(fit.krige_core(lp, Xp))
            keep.check("krige_core, max_rows = %d" % max_rows)
    finally:
        fit.close()
    st, qf = outs[0]
    _report("held-factor kriging", n, "against predict_core: stochastic %.2e quadform %.2e"
            % (_inf(st - want[0]) / _inf(want[0]), _inf((qf - want[1]) / want[1])))
    _assert_close(outs[0], want, KRIGE_TOL)
    for other in outs[1:]:
        assert np.array_equal(other[0], st) and np.array_equal(other[1], qf), "the chunking changed the bits"


@sizes
def test_joint_prediction(monkeypatch, n):
    """krige_joint covariance and three draws on the 70 rows against tests/krige_joint_reference.py on the oracle's matrices
    (the factor route, what the device computes; PARITY of max diag and of max |draw|: test_joint_against_oracle) and against
    the joint factorisation on the same handle (sim_cond_core: draws 1e-10, cov KRIGE_TOL of max diag:
    test_joint_matches_the_joint_factorisation); the stochastic part has the bits of krige_core; the covariance is symmetric to
    the bit; a repeated call gives the same bits."""
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    m = M_PRED
    E = np.random.default_rng(n).standard_normal((m, 3))
    fit = _fit(monkeypatch, n)
    try:
        keep = _Unchanged(fit, th)
        unit = fit.sim_cond_core(th, lp, Xp, lp, np.hstack([np.eye(m), E, np.zeros((m, 1))]))
        keep.check("sim_cond_core")
        fit.krige_prepare(th, max_rows=64)
        st0, qf0 = fit.krige_core(lp, Xp)
        st, cov, sims = fit.krige_joint_core(lp, Xp, iiderrors=E)
        keep.check("krige_joint_core")
        again = fit.krige_joint_core(lp, Xp, iiderrors=E)
    finally:
        fit.close()
    S2, C, Suu = KJ.matrices(O, th, locs, X, lp, Xp, lp, wl.SMOOTH_LIMITS)
    cov_ref = KJ.cov_trsm(S2, C, Suu)
    mu_ref = Xp @ th["mean"] + KJ.stochastic(S2, C, X, z[:, 0], th["mean"])
    want = KJ.draws(np.linalg.cholesky(cov_ref), E, mu_ref)
    top = float(np.max(np.diag(cov_ref)))
    e_cov, e_sims = _inf(cov - cov_ref) / top, _inf(sims - want) / _inf(want)
    e_st = _inf(Xp @ th["mean"] + st - mu_ref) / _inf(mu_ref)
    same, mu = unit[:, m:m + 3], unit[:, m + 3]
    L = np.tril(unit[:, :m] - mu[:, None])
    d_sims, d_cov = _inf(sims - same) / _inf(same), _inf(cov - L @ L.T) / float(np.max(np.diag(cov)))
    diag = 1 / np.exp(-(Xp @ th["std.dev"])) + np.exp(Xp @ th["nugget"])
    e_qf = _inf((np.diag(cov) - (diag - qf0)) / diag)
    _report("joint prediction", n, "reference: cov %.2e sims %.2e mean %.2e; joint factorisation: sims %.2e cov %.2e; diag against "
            "quadform %.2e" % (e_cov, e_sims, e_st, d_sims, d_cov, e_qf))
    assert np.array_equal(st, st0), "the stochastic part is krige_core's"
    assert np.array_equal(cov, cov.T)
    assert all(np.array_equal(a, b) for a, b in zip(again, (st, cov, sims)))
    assert e_cov <= PARITY and e_sims <= PARITY and e_st <= PARITY
    assert _inf(mu - (Xp @ th["mean"] + st)) <= KRIGE_TOL * _inf(mu)
    assert d_sims <= 1e-10 and d_cov <= KRIGE_TOL
    assert e_qf <= 1e-12                             # (test_joint_is_consistent_with_krige_core)


# --------------------------------------------------------------------------- n = p: no error contrasts
def test_fisher_reml_without_error_contrasts(monkeypatch):
    """n = p = 1: the projector P = Sigma^-1 - Sigma^-1 X (X' Sigma^-1 X)^-1 X' Sigma^-1 is zero, there are no error contrasts
    and the REML information is the zero matrix.  The entry does not refuse: it returns status 0 and the ALL-ZERO matrix, equal
    to the reference's (fisher_reml_reference.info_projector gives 0.0 in every entry here).  (Before this test the entry
    returned the square of the rounding error the projector kept: largest entry 1.23e-32 on MI355X.)  The value's bits
    survive the call; a repeated call gives the same."""
    locs, X, th, z, lp, Xp, S, Rz = problem(1)
    from cocons_amd import host, workloads as wl
    Sg, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, _units(1))
    ref = RR.info_projector(Sg, Sa, X, R)
    fit = _fit(monkeypatch, 1)
    try:
        keep = _Unchanged(fit, th)
        info = fit.fisher_reml_core(th, _units(1))
        keep.check("fisher_reml_core at n = p")
        again = fit.fisher_reml_core(th, _units(1))
    finally:
        fit.close()
    _report("fisher reml, n = p", 1, "largest entry %.2e (the reference's %.2e)" % (_inf(info), _inf(ref)))
    assert info.shape == (6, 6)
    assert np.all(ref == 0.0) and np.all(info == 0.0) and np.all(again == 0.0)


# --------------------------------------------------------------------------- sort on, sort off
@pytest.mark.parametrize("n", SORT_OFF_SIZES)
def test_sort_off_agrees_with_sort_on(monkeypatch, n):
    """COCONS_SPATIAL_SORT=0 on sites in no spatial order (n = 65: the smallest handle the sort rearranges; 129: two tiles with
    the largest front padding): leave-one-out and two-fold errors and variances (CV_BOUND) and the kriging rows (KRIGE_TOL)
    agree between the two handles and with the references, observation by observation in the caller's order; so do the
    information matrices (FISHER_TOL), which no order enters."""
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    p = X.shape[1]
    res = {}
    for sort in (True, False):
        fit = _fit(monkeypatch, n, sort=sort)
        try:
            keep = _Unchanged(fit, th)
            out = [fit.cv_core(th), fit.cv_core(th, _folds(n)["two"])]
            keep.check("cv_core")
            fit.krige_prepare(th, max_rows=64)
            out.append(fit.krige_core(lp, Xp))
            out.append(fit.predict_core(th, lp, Xp))
            out.append(fit.fisher_core(th, _units(p)))
            out.append(fit.fisher_reml_core(th, _units(p)))
            keep.check("the entries")
            res[sort] = out
        finally:
            fit.close()
    on, off = res[True], res[False]
    text = []
    for k, layout in enumerate(("loo", "two")):
        ge, gv = CV.gaps(off[k][0], off[k][1], on[k][0], on[k][1])
        re, rv = CV.gaps(off[k][0], off[k][1], *_ref_cv(n, layout))
        text.append("%s sort off against sort on gap_e %.2e gap_v %.2e, against brute force %.2e %.2e" % (layout, ge, gv, re, rv))
        assert max(ge, gv, re, rv) <= CV_BOUND, (layout, ge, gv, re, rv)
    text.append("kriging rows stochastic %.2e quadform %.2e" % (_inf(off[2][0] - on[2][0]) / _inf(on[2][0]),
                                                                 _inf((off[2][1] - on[2][1]) / on[2][1])))
    gi, gr = FR.metric(off[4][0], on[4][0]), FR.metric(off[5], on[5])
    text.append("information %.2e REML %.2e" % (gi, gr))
    _report("sort off", n, "; ".join(text))
    _assert_close(off[2], on[2], KRIGE_TOL)
    _assert_close(off[2], off[3], KRIGE_TOL)
    assert gi <= FISHER_TOL and gr <= FISHER_TOL
    assert FR.metric(off[4][0], R * _ref_fisher(n)[0]) <= FISHER_TOL and FR.metric(off[5], R * _ref_fisher(n)[1]) <= FISHER_TOL
