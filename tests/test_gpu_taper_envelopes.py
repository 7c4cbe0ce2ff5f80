"""Every entry of a tapered fit on band envelopes that are NOT flat -- wide in one place and at the floor in another (three
clusters among scattered sites), a clique laid out by the caller (columns eight tiles tall), a diagonal matrix, a chain, a
hub of stored zeros (W = nt - 1 packed, W = nt unpacked) and one stored zero far from the diagonal (the widest skew that
still packs) -- tests/taper_envelope_cases.py, seven named cases -- and on bands wider than eight tile rows: two flat bands of
W = 10 (flat9; flat10_long, twenty tile columns, the ring wraps twice) and a clique of 1300 sites laid out first (tall: column
0 twelve tile rows tall; tall_rcm, the library's order).  tests/test_taper_envelope_cases.py shows on the CPU that the far
tiles of those four matter to the answers held here; tests/golden/WIDE_BANDS_REPORT.md has the measured gaps.  flat10_long's
numpy references are expensive, so it runs the entries whose reference is S and one factorisation (no gradient, selected
inverse or exact Fisher information).

Every case ASSERTS the envelope it claims from what the handle reports: nt and W of krige_taper_info() equal the restated
rule (taper_envelope_cases.envelope_of) applied to the order the handle reports, the case's shape property holds for that
envelope, and the buffer is packed or not as cocons_debug_fit_memory shows.  A changed ordering or envelope rule makes these
tests say so.  The entries -- value and parts, gradient, selected inverse, Fisher information, leave-one-out, prediction,
held-factor kriging, simulation -- are then held against the independent references the suite has for each, at the tolerance
of the existing test of the same entry against the same reference (named at every comparison; none is loosened).  Every
test prints its worst errors.  References are computed once per case; what does not depend on the order of the
observations is computed once for a case and its twin in the caller's order."""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
import fisher_taper_reference as FT  # noqa: E402
import grad_taper_reference as GT  # noqa: E402
import krige_taper_joint_reference as KJ  # noqa: E402
import taper_envelope_cases as TE  # noqa: E402
from test_gpu_cv_taper import BOUND as CV_BOUND  # noqa: E402
from test_gpu_fisher_taper import TOL as FISHER_TOL  # noqa: E402
from test_gpu_grad_taper import _fit_memory, _inf, _selinv  # noqa: E402
from test_gpu_krige_taper import ROUTE_TOL  # noqa: E402
from test_gpu_krige_taper_joint import TOL_COV, TOL_SIMS, TOL_STOCHASTIC  # noqa: E402
from test_gpu_parity import N2LL_RTOL  # noqa: E402
from test_gpu_sim_taper import TOL as SIM_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

SL = TE.SMOOTH_LIMITS
LONG = "flat10_long"                  # no gradient, selected inverse or exact Fisher information (module docstring)
ENTRIES = ["clusters", "clusters_caller", "hub", "hub_caller", "lshape", "islands", "flat9", "tall", "tall_rcm"]
WITH_CHAIN = ENTRIES + ["chain"]
LAYOUTS = ["clusters", "hub", "lshape", "flat9", "tall", LONG]
WIDE = ["flat9", LONG, "tall", "tall_rcm"]
BRUTE_FOLDS = 64                      # leave-one-out by brute force above n = 1500: about this many refits
LAM = (0.1, 0.2, 0.3)                 # the penalty of test_taper_objective_vs_oracle

# The bound between the two device routes of the sparse prediction, ROUTE_TOL = 4 x 1.912e-14, is four times the worst
# difference measured on uniform sites (cond(S) of a few hundred).  clusters_caller (cond(S) = 2.0e4) measures 1.065e-13
# between the routes on MI355X, above it.  The reference of that comparison alone exceeds the bound there: against a
# long-double solve (oracle.chol_ld, Y = L^-1 [C' | resid] and the products summed in long double), in units of the largest
# stochastic value, the one-shot route the held factor is compared with stands at 1.656e-13, the held-factor route itself at
# 1.159e-13, numpy's double Cholesky with two triangular solves at 2.129e-13 and numpy.linalg.solve (the oracle) at 5.9e-14;
# the quadratic forms at 1.9e-15 and 1.8e-15.  For this case alone the bound is ten times the error of the route compared
# against, the margin the suite's long-double comparisons leave.  (clusters, the same matrix in the library's order: routes
# 2.77e-14 apart, each 1.30e-13 from long double; it keeps ROUTE_TOL.)
ROUTE_TOL_OF = {"clusters_caller": 10 * 1.656e-13}
SWITCHES = ("COCONS_TAPER_RCM", "COCONS_TAPER_PACKED", "COCONS_TAPER_BAND")


# --------------------------------------------------------------------------- handles and their shape
def _fit(monkeypatch, p, **env):
    """A handle of case p: the caller's order where the case says so, the buffer layout `env` asks for (the variables are read
    when the handle is created)."""
    import cocons_amd as ca
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if not p.rcm:
        monkeypatch.setenv("COCONS_TAPER_RCM", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return ca.CoconsTaperFit(p.locs, p.X, p.z, SL, *p.ref_taper)


def _assert_shape(fit, p, band=True):
    """The case's row of the table from what the handle reports; returns (order, nt, hi, W)."""
    order = fit.order()
    nt, hi, W, packed = TE.envelope_of(p.n, p.ref_taper[0], p.ref_taper[1], order)
    TE.assert_shape(p.name, nt, hi, W, packed)
    if not p.rcm:
        assert np.array_equal(order, np.arange(1, p.n + 1)), "the caller's order was not kept"
    info = fit.krige_taper_info()
    assert info["n"] == p.n and info["nt"] == nt, (info, nt)
    assert info["W"] == (W if band else nt), (info, W, (hi - np.arange(nt)).tolist())
    return order, nt, hi, W


def _theta_vector(th):
    """(optimiser vector with the mean free, par.pos) of a theta list: test_taper_handle_with_many_realisations"""
    from cocons_amd import workloads as wl
    pp = wl.par_pos_full()
    pp["mean"] = [True] * 3
    return np.r_[th["mean"], wl.theta_vector_from_lists(th, wl.par_pos_full())], pp


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _bad_thetas(th):
    """a NaN parameter and a matrix that is not positive definite (test_taper_handle_recovers_after_failed_evaluation)"""
    nan = OrderedDict((k, np.array(v, dtype=float)) for k, v in th.items())
    nan["std.dev"][0] = np.nan
    npd = OrderedDict((k, np.array(v, dtype=float)) for k, v in th.items())
    npd["std.dev"][0] = -np.inf
    npd["nugget"][0] = -np.inf
    return nan, npd


# --------------------------------------------------------------------------- references, once per case
@functools.lru_cache(maxsize=None)
def _ref_grad(base):
    """tests/grad_taper_reference.py at the case's theta: (f, parts, grad_logdet, grad_quad, grad_mean); sums over all
    observations, the same for a case and its twin in another order"""
    from cocons_amd.host import theta_table
    p = TE.problem(base)
    out = GT.neg2loglik_taper_grad(theta_table(p.theta), p.theta["mean"], p.locs, p.X, p.z, SL, p.ref_taper)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_matrix(base):
    """(S of tests/grad_taper_reference.py, the lower triangle mirrored as the library reads it; R = z - X mean)"""
    from cocons_amd.host import theta_table
    p = TE.problem(base)
    S, _ = GT.taper_matrix(theta_table(p.theta), p.locs, p.X, SL, p.ref_taper)
    out = (np.tril(S) + np.tril(S, -1).T, p.z - (p.X @ p.theta["mean"])[:, None])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_value(base):
    """(f, parts) as grad_taper_reference.neg2loglik_taper_grad states them.  flat10_long: from S and one factorisation, the
    lines of that function that give f and parts, without its gradient (20 s at n = 2433)."""
    if base != LONG:
        return _ref_grad(base)[:2]
    from scipy import linalg
    p = TE.problem(base)
    S, R = _ref_matrix(base)
    cf = linalg.cho_factor(S, lower=True)
    half_logdet = float(np.sum(np.log(np.diag(cf[0]))))
    quads = np.sum(R * linalg.cho_solve(cf, R), axis=0)
    parts = np.concatenate([[half_logdet], quads])
    parts.setflags(write=False)
    return R.shape[1] * (p.n * np.log(2 * np.pi) + 2 * half_logdet) + float(np.sum(quads)), parts


@functools.lru_cache(maxsize=None)
def _ref_oracle_values(base):
    """the oracle's objective with the penalty, its Profile form, and the plain value at the shifted theta"""
    from oracle import oracle as O
    O.build()
    p = TE.problem(base)
    tv, pp = _theta_vector(p.theta)
    tv2, _ = _theta_vector(TE.shifted(p.theta))
    args = (p.ref_taper, p.locs, p.X, SL, p.z, p.n)
    return (O.GetNeg2loglikelihoodTaper(tv, pp, *args, LAM), O.GetNeg2loglikelihoodTaperProfile(tv, pp, *args, LAM),
            O.GetNeg2loglikelihoodTaper(tv2, pp, *args, (0.0, 0.0, 0.0)))


@functools.lru_cache(maxsize=None)
def _oracle_matrix(name):
    """S of the oracle on the case's pattern, in the caller's order (test_gpu_sim_taper._S)"""
    from oracle import oracle as O
    from test_gpu_sim_taper import _S
    O.build()
    p = TE.problem(name)
    S = _S(O, p.theta, p.locs, p.X, p.ref_taper)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _ref_fisher(base):
    """(I at r = 1, X' S^-1 X) for the standard directions: tests/fisher_taper_reference.py; for the wide cases also S and
    the direction matrices themselves (what the probe mode's numpy sweep runs on)"""
    from cocons_amd.host import theta_table
    p = TE.problem(base)
    S, Sa = FT.direction_matrices(theta_table(p.theta), p.locs, p.X, SL, p.ref_taper, FT.standard_directions(3))
    out = (FT.info_whiten(S, Sa, 1), FT.info_mean(S, p.X, 1)) + ((S, Sa) if base in WIDE else ())
    for a in out:
        a.setflags(write=False)
    return out


def _brute_stride(base):
    """every 4th observation, every 8th above n = 1000; above n = 1500, where one refit costs a second, the stride that
    leaves about BRUTE_FOLDS refits (27 at n = 1665: 62 of them; 30 at n = 1869: 63); flat10_long: no refit at all (0)"""
    n = TE.problem(base).n
    if base == LONG:
        return 0
    return -(-n // BRUTE_FOLDS) if n > 1500 else (8 if n > 1000 else 4)


@functools.lru_cache(maxsize=None)
def _ref_cv(base):
    """(e, var of cv_reference.cv_kroute for every observation; idx, e, var of cv_reference.cv_brute for every
    _brute_stride-th observation) on the dense S of grad_taper_reference, as test_gpu_cv_taper._reference.  Brute force is one Cholesky
    of order n - 1 per observation it predicts -- 19 s for the 1281 of clusters -- so it predicts a stride of them: each of
    these is a fold of its own, all the others share one fold whose result is dropped, and cv_brute's answer for a fold of
    one is the leave-one-out prediction whatever the other folds are.  The stride runs over the caller's order, which the
    handle's order scatters over every tile column.  Every observation is held to the route through the dense inverse, which
    test_leave_one_out_vs_reference uses above n = 700 and tests/test_cv_reference.py pins to brute force."""
    p = TE.problem(base)
    S, R = _ref_matrix(base)
    stride = _brute_stride(base)
    idx = np.arange(0, p.n, stride) if stride else np.zeros(0, dtype=int)
    lab = np.full(p.n, -1)
    lab[idx] = idx
    eb, vb = CV.cv_brute(S, R, lab) if idx.size else (np.zeros((0, 1)), np.zeros(0))
    out = CV.cv_kroute(S, R, np.arange(p.n)) + (idx, eb[idx], vb[idx])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_predict(name):
    from oracle import oracle as O
    O.build()
    p = TE.problem(name)
    out = O.cocoPredict_sparse(p.theta, p.locs, p.lp, p.X, p.Xp, SL, p.z[:, 0], p.ref_taper, p.pred_taper)
    for a in out.values():
        a.setflags(write=False)
    return out


def _check_predict(tag, p, st, qf, want):
    """the bounds of test_taper_predict_vs_oracle (test_chunked_predict_vs_oracle uses the same)"""
    from cocons_amd.host import _sparse_predict_tail
    got = _sparse_predict_tail(p.theta, p.Xp, st, qf, "pred")
    e_sys = _inf(got["systematic"] - want["systematic"]) / _inf(want["systematic"])
    e_st = _inf(got["stochastic"] - want["stochastic"]) / _inf(want["stochastic"])
    e_sd = _inf(got["sd.pred"] - want["sd.pred"]) / _inf(want["sd.pred"])
    print("%s %s: systematic %.2e stochastic %.2e sd.pred %.2e" % (p.name, tag, e_sys, e_st, e_sd))
    assert np.allclose(got["systematic"], want["systematic"], rtol=1e-13, atol=0)
    assert e_st < 1e-10
    assert e_sd < 1e-9
    assert got["stochastic"][p.special[1]] == 0.0                  # the row without neighbours: exactly zero


# --------------------------------------------------------------------------- shape first
@pytest.mark.parametrize("name", TE.NAMES)
def test_shape_reported_by_the_handle(monkeypatch, name):
    """nt and W of krige_taper_info() after krige_taper_prepare equal the restated rule on the order the handle reports; the
    case's shape holds; a fresh handle's buffer has W + 1 tile rows per tile column when packed and nt + 1 when not (one tile
    row under the matrix for the r + p <= 128 right-hand sides), as cocons_debug_fit_memory reports it."""
    p = TE.problem(name)
    fit = _fit(monkeypatch, p)
    try:
        mem = _fit_memory(fit)
        fit.krige_taper_prepare(p.theta, max_rows=64)
        info = fit.krige_taper_info()
        order, nt, hi, W = _assert_shape(fit, p)
    finally:
        fit.close()
    packed = W < nt
    print("%s: n %d nt %d W %d packed %s hi - c %s, leading dimension %d" % (name, p.n, nt, W, packed,
                                                                           (hi - np.arange(nt)).tolist(), mem[3]))
    assert info["prepared"] and info["rows"] == 64
    assert mem[3] == ((W if packed else nt) + 1) * TE.TILE, mem
    assert mem[0] == 8 * mem[3] * nt * TE.TILE, mem
    if name == "hub_caller":
        assert not packed and mem[3] == (nt + 1) * TE.TILE


# --------------------------------------------------------------------------- entries
@pytest.mark.parametrize("name", WITH_CHAIN + [LONG])
def test_value_and_parts(monkeypatch, name):
    """GetNeg2loglikelihoodTaper and its Profile form against the oracle (1e-8: test_taper_objective_vs_oracle); value and
    parts of neg2loglik_core against tests/grad_taper_reference.py (value 1e-9: test_value_and_gradient_vs_reference; every
    entry of parts 1e-9: tests/test_gpu_rhs_layouts.py); a second evaluation at a shifted theta on the same handle against the
    oracle (1e-8); then the first theta again: the first call's bits -- re-zeroing a varying envelope leaves no tile behind."""
    import cocons_amd as ca
    p = TE.problem(name)
    want, wantp, want2 = _ref_oracle_values(p.base)
    f, rparts = _ref_value(p.base)
    tv, pp = _theta_vector(p.theta)
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        args = (p.ref_taper, p.locs, p.X, SL, p.z, p.n, LAM)
        got = ca.GetNeg2loglikelihoodTaper(tv, pp, *args, fit=fit)
        gotp = ca.GetNeg2loglikelihoodTaperProfile(tv, pp, *args, fit=fit)
        v0 = fit.neg2loglik_core(p.theta)
        v2 = fit.neg2loglik_core(TE.shifted(p.theta))
        v1 = fit.neg2loglik_core(p.theta)
    finally:
        fit.close()
    e = (abs(got - want) / abs(want), abs(gotp - wantp) / abs(wantp), abs(v0[0] - f) / abs(f),
         _inf(v0[1] / rparts - 1), abs(v2[0] - want2) / abs(want2))
    print("%s: objective %.2e Profile %.2e | value %.2e parts %.2e against the numpy statement | shifted theta %.2e" % ((name,) + e))
    assert e[0] <= N2LL_RTOL and e[1] <= N2LL_RTOL and e[4] <= N2LL_RTOL
    assert e[2] <= 1e-9 and e[3] <= 1e-9
    assert v1[0] == v0[0] and np.array_equal(v1[1], v0[1]), "the first theta again"
    assert v2[0] != v0[0]


@pytest.mark.parametrize("name", WITH_CHAIN)
def test_gradient(monkeypatch, name):
    """neg2loglik_grad_core as test_value_and_gradient_vs_reference holds it: value and parts equal the value entry's (1e-12),
    grad_theta, grad_quad and grad_mean against the numpy statement (1e-7 of each one's largest component), value 1e-9, the
    scaling identity (1e-9 r n), two calls the same bits, the value call afterwards the bits it gave before."""
    p = TE.problem(name)
    f, rparts, rl, rq, rm = _ref_grad(p.base)
    r = p.z.shape[1]
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        v0, p0 = fit.neg2loglik_core(p.theta)
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(p.theta)
        v1, p1 = fit.neg2loglik_core(p.theta)
        again = fit.neg2loglik_grad_core(p.theta)
    finally:
        fit.close()
    assert v1 == v0 and np.array_equal(p1, p0)
    assert again[0] == v and _same(again[1:], (parts, gt, gq, gm))
    assert np.all(gt[2] == 0) and np.all(gt[3] == 0) and np.all(gq[2] == 0) and np.all(gq[3] == 0)
    errs = [_inf(g - w) / _inf(w) for g, w in ((gt, rl + rq), (gq, rq), (gm, rm))]
    ident = gt[0, 0] + gt[5, 0] - (r * p.n - float(np.sum(parts[1:])))
    print("%s: value %.2e (value entry %.2e, parts %.2e) grad_theta %.2e grad_quad %.2e grad_mean %.2e identity %.2e of r n"
          % (name, abs(v - f) / abs(f), abs(v - v0) / abs(v0), _inf(parts - p0) / _inf(p0), errs[0], errs[1], errs[2],
             abs(ident) / (r * p.n)))
    assert abs(v - v0) <= 1e-12 * abs(v0)
    assert _inf(parts - p0) <= 1e-12 * _inf(p0)
    assert max(errs) <= 1e-7, errs
    assert abs(v - f) <= 1e-9 * abs(f)
    assert abs(ident) <= 1e-9 * r * p.n


@pytest.mark.parametrize("name", ENTRIES)
def test_selected_inverse(monkeypatch, name):
    """cocons_debug_taper_selinv at every stored entry, stored zeros included (hub: they reach as far from the diagonal as the
    matrix goes, so the tallest columns of Z are read back), against numpy.linalg.inv of the oracle's matrix: 1e-10 of
    max |S^-1| (test_selected_inverse_vs_dense_inverse)."""
    p = TE.problem(name)
    ci, rp, ent = p.ref_taper
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        got, _ = _selinv(fit, p.theta, ci.size)
        got2, _ = _selinv(fit, p.theta, ci.size)
    finally:
        fit.close()
    rows = np.repeat(np.arange(p.n), np.diff(rp))
    want = np.linalg.inv(_oracle_matrix(name))[rows, ci - 1]
    zero = ent == 0.0
    print("%s: selected inverse %.2e of max |S^-1| = %.3g over %d stored entries (%d stored zeros: %.2e)"
          % (name, _inf(got - want) / _inf(want), _inf(want), ci.size, int(zero.sum()),
             _inf((got - want)[zero]) / _inf(want) if zero.any() else 0.0))
    assert _inf(got - want) <= 1e-10 * _inf(want)
    assert np.array_equal(got, got2)


@pytest.mark.parametrize("name", ENTRIES)
def test_fisher_exact_mode(monkeypatch, name):
    """fisher_core, exact mode, the standard directions, in chunks of 64 probe rows: the gap to tests/
    fisher_taper_reference.py within 1e-7 and info_mean within 1e-10 (test_exact_mode_against_reference); max_rows = 0 gives
    the same bits.  clusters: the mirrored envelope of the flipped factor is not the envelope, so the sweep's second set of
    tables differs from its first."""
    p = TE.problem(name)
    R, Rm = _ref_fisher(p.base)[:2]
    r = p.z.shape[1]
    dirs = FT.standard_directions(3)
    fit = _fit(monkeypatch, p)
    try:
        order, nt, hi, W = _assert_shape(fit, p)
        info, info_mean = fit.fisher_core(p.theta, dirs, max_rows=64)
        info0, info_mean0 = fit.fisher_core(p.theta, dirs, max_rows=0)
    finally:
        fit.close()
    hib = TE.mirrored_envelope(hi)
    if name == "clusters":
        assert not np.array_equal(hib, hi), (hib, hi)
    gap = FT.metric(info, r * R)
    gm = _inf(info_mean - r * Rm) / _inf(r * Rm)
    print("%s: exact mode gap %.2e info_mean %.2e (envelope %s, mirrored %s)"
          % (name, gap, gm, (hi - np.arange(nt)).tolist(), (hib - np.arange(nt)).tolist()))
    assert gap <= FISHER_TOL
    assert gm <= 1e-10
    assert np.array_equal(info, info.T) and np.array_equal(info_mean, info_mean.T)
    assert np.array_equal(info0, info) and np.array_equal(info_mean0, info_mean), "the chunk size changed the bits"


@pytest.mark.parametrize("name", ENTRIES + [LONG])
def test_leave_one_out(monkeypatch, name):
    """cv_core against cv_reference.cv_brute at every 8th or 4th observation (the wide cases: _brute_stride; flat10_long: none)
    and against cv_reference.cv_kroute at every one (_ref_cv): gap_e and gap_v within 1e-8
    (test_leave_one_out_vs_reference); two calls give the same bits."""
    p = TE.problem(name)
    e, var, idx, eb, vb = _ref_cv(p.base)
    where = np.empty(p.n, dtype=int)
    where[p.perm] = np.arange(p.n)                                 # the base's observation i is observation where[i] here
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        got = fit.cv_core(p.theta)
        again = fit.cv_core(p.theta)
    finally:
        fit.close()
    assert got[0].shape == p.z.shape and got[1].shape == (p.n,)
    ge, gv = CV.gaps(got[0], got[1], e[p.perm], var[p.perm])
    assert idx.size or name == LONG
    be, bv = CV.gaps(got[0][where[idx]], got[1][where[idx]], eb, vb) if idx.size else (0.0, 0.0)
    re, rv = CV.gaps(e[idx], var[idx], eb, vb) if idx.size else (0.0, 0.0)
    print("%s: leave-one-out gap_e %.2e gap_v %.2e at all %d observations (dense inverse), %.2e %.2e at %d of them (brute "
          "force; the two references there: %.2e %.2e); var %.3g .. %.3g" % (name, ge, gv, p.n, be, bv, idx.size, re, rv,
                                                                          var.min(), var.max()))
    assert ge <= CV_BOUND and gv <= CV_BOUND
    assert be <= CV_BOUND and bv <= CV_BOUND
    assert _same(got, again)


@pytest.mark.parametrize("name", ENTRIES + [LONG])
def test_prediction(monkeypatch, name):
    """predict_core against the oracle's cocoPredict_sparse at the bounds of test_taper_predict_vs_oracle; the row without
    neighbours gives a stochastic part of exactly 0; the objective's bits survive the prediction's larger border."""
    p = TE.problem(name)
    want = _ref_predict(name)
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        v0 = fit.neg2loglik_core(p.theta)
        st, qf = fit.predict_core(p.theta, p.lp, p.Xp, p.pred_taper)
        v1 = fit.neg2loglik_core(p.theta)
    finally:
        fit.close()
    _check_predict("predict_core", p, st, qf, want)
    assert qf[p.special[1]] == 0.0
    assert v1[0] == v0[0] and np.array_equal(v1[1], v0[1])


@pytest.mark.parametrize("name", WITH_CHAIN + [LONG])
def test_held_factor_kriging(monkeypatch, name):
    """krige_taper_prepare(max_rows = 64), krige_taper_core on the 200 rows (four chunks, the last one of 8 rows): against
    predict_core on the same handle (4 x 1.912e-14 of the largest value: test_matches_the_one_shot_route; clusters_caller:
    1.656e-12, ten times the one-shot route's own distance from a long-double solve, see ROUTE_TOL_OF) and against the
    oracle (test_chunked_predict_vs_oracle); one chunk gives the same bits; so do the three whole 64-row blocks permuted.
    W = 6, 7 and 8 do not divide nt = 11 and 8: the ring wraps where no other test has it wrap.  The wide cases (W = 10, 11
    and 12 of nt = 14, 15 and 20) keep ROUTE_TOL: an update step there has up to W (W + 1) / 2 = 78 tiles, and the slot of
    tile column I is I mod W with W > 8."""
    from test_gpu_krige_taper import _err
    p = TE.problem(name)
    want = _ref_predict(name)
    fit = _fit(monkeypatch, p)
    try:
        order, nt, hi, W = _assert_shape(fit, p)
        one_shot = fit.predict_core(p.theta, p.lp, p.Xp, p.pred_taper)
        fit.krige_taper_prepare(p.theta, max_rows=64)
        assert fit.krige_taper_info()["rows"] == 64
        got = fit.krige_taper_core(p.lp, p.Xp, p.pred_taper)
        idx = np.concatenate([np.arange(64 * b, 64 * b + 64) for b in (2, 0, 1)] + [np.arange(192, TE.M_PRED)])
        moved = fit.krige_taper_core(p.lp[idx], p.Xp[idx], TE.take_rows(p.pred_taper, idx))
        fit.krige_taper_prepare(p.theta, max_rows=256)
        assert fit.krige_taper_info()["rows"] == 256
        whole = fit.krige_taper_core(p.lp, p.Xp, p.pred_taper)
    finally:
        fit.close()
    e = _err(got, one_shot)
    print("%s (nt %d, W %d): held factor against the one-shot route: stochastic %.3e quadform %.3e" % (name, nt, W, e[0], e[1]))
    _check_predict("krige_taper_core", p, got[0], got[1], want)
    assert max(e) <= ROUTE_TOL_OF.get(name, ROUTE_TOL), e
    assert got[0][p.special[1]] == 0.0 and got[1][p.special[1]] == 0.0
    assert _same(whole, got), "one chunk"
    assert np.array_equal(moved[0], got[0][idx]) and np.array_equal(moved[1], got[1][idx]), "blocks of rows permuted"


PIVOTED = ("clusters", "flat9", "tall")


@pytest.mark.parametrize("name", ENTRIES + [LONG])
def test_simulation(monkeypatch, name):
    """sim_core in the handle's own order with 65 draws (one more than a pass of band_trmm_kernel) against
    numpy.linalg.cholesky(S[order][:, order]) @ E + trend: 1e-10 of the largest value (test_fast_route_own_order).  clusters,
    flat9 and tall: also a pivot that is neither the handle's order nor the identity (test_draw_equal_route_pivot, the same
    bound) -- the twin handle in the pivot's order has an envelope of its own (a random order: no band at all)."""
    from test_gpu_sim_taper import _want
    p = TE.problem(name)
    S = _oracle_matrix(name)
    rng = np.random.default_rng(65 + p.n)
    E = rng.standard_normal((p.n, 65))
    trend = p.X @ p.theta["mean"]
    fit = _fit(monkeypatch, p)
    try:
        order = _assert_shape(fit, p)[0]
        got = fit.sim_core(p.theta, E)
        again = fit.sim_core(p.theta, E)
        if name in PIVOTED:
            piv = (rng.permutation(p.n) + 1).astype(np.int32)
            assert not np.array_equal(piv, order) and not np.array_equal(piv, np.arange(1, p.n + 1))
            got_piv = fit.sim_core(p.theta, E, pivot=piv)
            own_after = fit.sim_core(p.theta, E)
    finally:
        fit.close()
    want = _want(S, order, E, trend)
    e = _inf(got - want) / _inf(want)
    print("%s: 65 draws in the handle's order %.2e" % (name, e))
    assert got.shape == (p.n, 65) and e <= SIM_TOL
    assert np.array_equal(got, again)
    if name in PIVOTED:
        want_piv = _want(S, piv, E, trend)
        e = _inf(got_piv - want_piv) / _inf(want_piv)
        print("%s: 65 draws with a caller's pivot %.2e" % (name, e))
        assert e <= SIM_TOL
        assert np.array_equal(own_after, got) and not np.array_equal(got_piv, got)


# --------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("name", LAYOUTS)
def test_buffer_layouts(monkeypatch, name):
    """COCONS_TAPER_PACKED=0 (the dense buffer, its band used) gives the packed default's bits in value, parts, gradient,
    prediction and kriging (test_taper_packed_band_buffer_equals_dense_buffer and test_buffer_layouts_give_the_same_bits claim
    it at W = 5; here W = 6, W = nt - 1 and, on flat9, tall and flat10_long, W = 10 and 12: a leading dimension of (W + 1) 128 =
1408 and 1664 rows).  COCONS_TAPER_BAND=0 (no envelope: another schedule) agrees in value (1e-12), parts
    (1e-12 of the largest) and gradient (1e-10 of the largest component of grad_theta), the bounds of
    test_buffer_layouts_and_orders_agree and test_value_and_gradient_vs_reference."""
    p = TE.problem(name)
    res, lda = {}, {}
    for layout, env in (("packed", {}), ("unpacked", {"COCONS_TAPER_PACKED": "0"}), ("noband", {"COCONS_TAPER_BAND": "0"})):
        fit = _fit(monkeypatch, p, **env)
        try:
            lda[layout] = _fit_memory(fit)[3]
            order, nt, hi, W = _assert_shape(fit, p, band=layout != "noband")
            out = list(fit.neg2loglik_core(p.theta)) + list(fit.neg2loglik_grad_core(p.theta))
            if layout != "noband":
                out += list(fit.predict_core(p.theta, p.lp, p.Xp, p.pred_taper))
                fit.krige_taper_prepare(p.theta, max_rows=64)
                out += list(fit.krige_taper_core(p.lp, p.Xp, p.pred_taper))
                out += list(fit.neg2loglik_core(p.theta))          # after the prediction regrew the rows under the matrix
            res[layout] = out
        finally:
            fit.close()
    assert lda["packed"] == (W + 1) * TE.TILE and lda["unpacked"] == lda["noband"] == (nt + 1) * TE.TILE, lda
    a, b, c = res["packed"], res["unpacked"], res["noband"]
    assert len(a) == len(b) == 13
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "output %d differs between the packed and the dense buffer" % k
    assert a[11] == a[0] and np.array_equal(a[12], a[1])
    e_v, e_p = abs(c[0] - a[0]) / abs(a[0]), _inf(c[1] - a[1]) / _inf(a[1])
    e_g = [_inf(c[k] - a[k]) / _inf(a[4]) for k in (4, 5, 6)]
    print("%s: no envelope against the packed band: value %.2e parts %.2e gradient %.2e %.2e %.2e" % ((name, e_v, e_p) + tuple(e_g)))
    assert e_v <= 1e-12 and e_p <= 1e-12
    assert max(e_g) <= 1e-10


# --------------------------------------------------------------------------- recovery on a wide envelope
def test_recovery_on_a_wide_envelope(monkeypatch):
    """clusters: a NaN theta and a theta whose matrix is not positive definite (the -Inf variance of
    test_taper_handle_recovers_after_failed_evaluation) each poison every tile the factorisation touches; the first theta
    afterwards gives the first call's bits, value and gradient: nothing is left in a column taller than the floor."""
    _recovery(monkeypatch, "clusters")


def test_recovery_on_a_tall_envelope(monkeypatch):
    """the same on tall: column 0 is twelve tile rows tall, and every one of them is poisoned and must come back clean"""
    _recovery(monkeypatch, "tall")


def _recovery(monkeypatch, name):
    import cocons_amd as ca
    p = TE.problem(name)
    nan, npd = _bad_thetas(p.theta)
    tv, pp = _theta_vector(p.theta)
    tv_nan = tv.copy()
    tv_nan[3] = np.nan
    args = (p.ref_taper, p.locs, p.X, SL, p.z, p.n, (0.0, 0.0, 0.0))
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        first = fit.neg2loglik_core(p.theta)
        g_first = fit.neg2loglik_grad_core(p.theta)
        for bad in (nan, npd):
            with pytest.raises(ca.CholeskyError):
                fit.neg2loglik_core(bad)
            again = fit.neg2loglik_core(p.theta)
            assert again[0] == first[0] and np.array_equal(again[1], first[1])
            with pytest.raises(ca.CholeskyError):
                fit.neg2loglik_grad_core(bad)
            g_again = fit.neg2loglik_grad_core(p.theta)
            assert g_again[0] == g_first[0] and _same(g_again[1:], g_first[1:])
        assert ca.GetNeg2loglikelihoodTaper(tv_nan, pp, *args, fit=fit) == 1e6
        again = fit.neg2loglik_core(p.theta)
        assert again[0] == first[0] and np.array_equal(again[1], first[1])
    finally:
        fit.close()
    f = _ref_grad(p.base)[0]
    print("%s: value after two poisoned evaluations %.2e against the numpy statement" % (name, abs(first[0] - f) / abs(f)))
    assert abs(first[0] - f) <= 1e-9 * abs(f)


# --------------------------------------------------------------------------- what the wide cases are the first to meet
@functools.lru_cache(maxsize=None)
def _uu(base):
    """the case's taper among its own prediction rows (the row without a neighbour holds its diagonal alone)"""
    p = TE.problem(base)
    out = TE.device_pattern(p.lp, p.lp, p.delta, TE.KIND_OF[base])
    for a in out:
        a.setflags(write=False)
    return out


def _dense(pattern, entries, nrow, ncol):
    ci, rp = np.asarray(pattern[0]), np.asarray(pattern[1])
    A = np.zeros((nrow, ncol))
    A[np.repeat(np.arange(nrow), np.diff(rp)), ci - 1] = entries
    return A


@functools.lru_cache(maxsize=None)
def _ref_joint(base):
    """The dense numpy statement of test_gpu_krige_taper_joint._reference on the case: (stochastic, S_uu, cov, mu, C); S_uu from
    the lower triangle of the uu pattern, mirrored; C the m x n cross-covariances on the prediction pattern."""
    from oracle import oracle as O
    O.build()
    p = TE.problem(base)
    uu, pt, th, m = _uu(base), p.pred_taper, p.theta, TE.M_PRED
    S = _oracle_matrix(base)
    C = _dense(pt, np.asarray(pt[2]) * O.cov_rns_taper_pred(th, p.locs, p.lp, p.X, p.Xp, pt[0], pt[1], SL), m, p.n)
    Su = np.tril(_dense(uu, np.asarray(uu[2]) * O.cov_rns_taper(th, p.lp, p.Xp, uu[0], uu[1], SL), m, m))
    Su = Su + np.tril(Su, -1).T
    SiCt = np.linalg.solve(S, C.T)
    st = (p.z[:, 0] - p.X @ th["mean"]) @ SiCt
    cov = Su - C @ SiCt
    out = (st, Su, (cov + cov.T) / 2, p.Xp @ th["mean"] + st, C)
    for a in out:
        a.setflags(write=False)
    return out


def _ring_schur(name, order, hi, W, depth):
    """tests/krige_taper_joint_reference.py (the ring of min(W + depth - 1, nt) slots, tile column I in slot I mod that) at the
    tile edge 128 on the dense numpy factor in the handle's order: S_uu - sum_g V_g V_g'"""
    p = TE.problem(name)
    assert np.array_equal(p.perm, np.arange(p.n))
    _, Su, _, _, C = _ref_joint(p.base)
    o = np.asarray(order) - 1
    nt = len(hi)
    Sp = np.eye(nt * TE.TILE)
    Sp[:p.n, :p.n] = _oracle_matrix(p.base)[np.ix_(o, o)]
    L = np.linalg.cholesky(Sp)
    stored = _dense(p.pred_taper, 1.0, TE.M_PRED, p.n)[:, o] != 0
    Co = C[:, o]
    rows_ci = [np.nonzero(stored[i])[0] for i in range(TE.M_PRED)]
    rows_val = [Co[i, rows_ci[i]] for i in range(TE.M_PRED)]
    return KJ.ring_schur(L, [int(h) for h in hi], TE.TILE, W, depth, rows_ci, rows_val, Su)[0]


@pytest.mark.parametrize("name", WIDE)
def test_joint_prediction(monkeypatch, name):
    """krige_taper_joint on the 200 prediction rows against the dense numpy statement of test_gpu_krige_taper_joint._reference
    at that file's bounds (TOL_COV, TOL_SIMS, TOL_STOCHASTIC; above 1e-10 a defect) and against the ring solve of tests/
    krige_taper_joint_reference.py on the numpy factor (TOL_COV): the covariance on all rows; covariance and three draws on
    the 199 rows off the observation (with the row on top of an observation the predictive covariance is singular, tests/
    golden/SIZES_REPORT.md: no draw is defined there).  The stochastic part has the bits of krige_taper_core
    (test_same_bits_as_apply); the covariance is symmetric to the bit; ring depths 1 and 3 (W and W + 2 slots: both wrap, the
    second at a modulus that is not W) give the default's bits."""
    from test_gpu_krige_taper_joint import _default_depth, _eq
    from taper_size_cases import sub_pattern
    p = TE.problem(name)
    uu = _uu(p.base)
    st_ref, Su, cov_ref, mu, _ = _ref_joint(p.base)
    rows = np.delete(np.arange(TE.M_PRED), p.special[2])
    sub_ref = cov_ref[np.ix_(rows, rows)]
    ev = np.linalg.eigvalsh(sub_ref)
    assert ev.min() > 0
    E = np.random.default_rng(70 + p.n).standard_normal((TE.M_PRED, 3))
    monkeypatch.delenv("COCONS_KRIGE_JOINT_DEPTH", raising=False)
    fit = _fit(monkeypatch, p)
    try:
        order, nt, hi, W = _assert_shape(fit, p)
        fit.krige_taper_prepare(p.theta)
        depth = _default_depth(fit, TE.M_PRED, monkeypatch)
        st0, qf0 = fit.krige_taper_core(p.lp, p.Xp, p.pred_taper)
        st, cov, none = fit.krige_taper_joint_core(p.lp, p.Xp, p.pred_taper, uu)
        sub = (p.lp[rows], p.Xp[rows], TE.take_rows(p.pred_taper, rows), sub_pattern(uu, rows))
        drawn = fit.krige_taper_joint_core(*sub, iiderrors=E[rows])
        depths = {}
        for d in ("1", "3"):
            monkeypatch.setenv("COCONS_KRIGE_JOINT_DEPTH", d)
            depths[d] = fit.krige_taper_joint_core(p.lp, p.Xp, p.pred_taper, uu)
        monkeypatch.delenv("COCONS_KRIGE_JOINT_DEPTH")
    finally:
        fit.close()
    assert none is None and W + 3 - 1 < nt, (W, nt)
    top = float(np.max(np.diag(cov_ref)))
    want = np.linalg.cholesky(sub_ref) @ E[rows] + mu[rows, None]
    e_cov = _inf(cov - cov_ref) / top
    e_ring = _inf(cov - _ring_schur(name, order, hi, W, 3)) / top
    e_sub = _inf(drawn[1] - sub_ref) / float(np.max(np.diag(sub_ref)))
    e_sims = _inf(drawn[2] - want) / _inf(want)
    e_st = _inf(st - st_ref) / _inf(st_ref)
    e_qf = _inf((np.diag(Su) - np.diag(cov)) - qf0) / top
    print("%s (nt %d, W %d, default depth %d): joint prediction cov %.3e (ring solve in numpy %.3e; 199 rows %.3e) sims %.3e "
          "stochastic %.3e diag against quadform %.3e (eigenvalues %.3e .. %.3e)"
          % (name, nt, W, depth, e_cov, e_ring, e_sub, e_sims, e_st, e_qf, ev.min(), ev.max()))
    assert np.array_equal(st, st0), "the stochastic part is krige_taper_core's"
    assert np.array_equal(drawn[0], st0[rows])
    assert np.array_equal(cov, cov.T) and np.array_equal(drawn[1], drawn[1].T)
    for d, b in depths.items():
        assert _eq(b, (st, cov, None)), "depth " + d
    assert st[p.special[1]] == 0.0 and np.count_nonzero(cov[p.special[1]]) == 1 and cov[p.special[1], p.special[1]] > 0
    assert max(e_cov, e_ring, e_sub, e_sims, e_st) <= 1e-10, "a defect, not a bound"
    assert e_cov <= TOL_COV and e_sub <= TOL_COV and e_sims <= TOL_SIMS and e_st <= TOL_STOCHASTIC, (e_cov, e_sub, e_sims, e_st)
    assert e_ring <= TOL_COV and e_qf <= TOL_COV, (e_ring, e_qf)


@pytest.mark.parametrize("name", TE.FLAT)
def test_device_pattern(monkeypatch, name):
    """The flat cases have no stored zero: their pattern is a function of delta.  CoconsTaperFit.from_delta reports the order,
    nt and W of the handle built from ref_taper and gives the bits of its value (test_create_taper_delta); the exported
    patterns are ref_taper and pred_taper, entries included (tests/test_gpu_pattern.py allows 16 x 2^-52 and measures 0; the
    cases' entries are evaluated in the device's order of operations); krige_taper_core_delta gives the bits of krige_taper_core
    fed the exported pattern (test_apply_delta_equals_apply_bit_for_bit), in chunks of 64 rows and in one."""
    import cocons_amd as ca
    p = TE.problem(name)
    kind = TE.KIND_OF[p.base]
    fit = _fit(monkeypatch, p)
    other = None
    try:
        order, nt, hi, W = _assert_shape(fit, p)
        other = ca.CoconsTaperFit.from_delta(p.locs, p.X, p.z, SL, p.delta, kind)
        info = other.krige_taper_info()
        assert np.array_equal(other.order(), order) and (info["nt"], info["W"]) == (nt, W), info
        v, va = fit.neg2loglik_core(p.theta), other.neg2loglik_core(p.theta)
        own = ca.taper_pattern(p.locs, p.delta, kind)
        exported = ca.taper_pattern(p.locs, p.delta, kind, newlocs=p.lp)
        dev = max(_inf(own[2] / p.ref_taper[2] - 1), _inf(exported[2] / p.pred_taper[2] - 1))
        print("%s (%s, delta %g, nt %d, W %d): %d + %d entries from the device, largest deviation from the case's %.3e"
              % (name, kind, p.delta, nt, W, own[0].size, exported[0].size, dev))
        got = {}
        for max_rows in (64, 0):
            fit.krige_taper_prepare(p.theta, max_rows=max_rows)
            got[max_rows] = (fit.krige_taper_core(p.lp, p.Xp, exported), fit.krige_taper_core_delta(p.lp, p.Xp, p.delta, kind),
                             fit.krige_taper_core(p.lp, p.Xp, p.pred_taper))
            assert fit.last_pattern_nnz == exported[0].size
    finally:
        fit.close()
        if other is not None:
            other.close()
    for mine, theirs in ((p.ref_taper, own), (p.pred_taper, exported)):
        assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
        assert np.array_equal(mine[2], theirs[2]), dev
    assert va[0] == v[0] and np.array_equal(va[1], v[1]), "from_delta: the value's bits"
    for max_rows, (fed, from_delta, mine) in got.items():
        assert _same(from_delta, fed), "krige_taper_core_delta, max_rows %d" % max_rows
        assert _same(mine, fed)
    assert _same(got[0][1], got[64][1])
    empty = np.nonzero(np.diff(p.pred_taper[1]) == 0)[0]
    assert p.special[1] in empty and np.all(got[64][1][0][empty] == 0.0) and np.all(got[64][1][1][empty] == 0.0)


PROBED = ["flat9", "tall"]            # (the numpy sweep costs 20 s a call at these sizes)


@pytest.mark.parametrize("nprobe", [64, 100])
@pytest.mark.parametrize("name", PROBED)
def test_fisher_probe_mode(monkeypatch, name, nprobe):
    """random +-1 probes through the handle's own order against the same probes through fisher_taper_reference.band_fisher with
    the handle's pivot: FISHER_TOL, info_mean 1e-10 (test_probe_mode_against_the_numpy_sweep, test_gpu_taper_sizes.
    test_fisher_probe_mode); 100 probes leave the second strip partly filled"""
    p = TE.problem(name)
    assert np.array_equal(p.perm, np.arange(p.n))
    _, Rm, S, Sa = _ref_fisher(p.base)
    r = p.z.shape[1]
    dirs = FT.standard_directions(3)
    P = np.random.default_rng(nprobe + p.n).integers(0, 2, size=(p.n, nprobe)) * 2.0 - 1.0
    fit = _fit(monkeypatch, p)
    try:
        pivot, nt, hi, W = _assert_shape(fit, p)
        info, info_mean = fit.fisher_core(p.theta, dirs, probes=P)
    finally:
        fit.close()
    want, _, rhi, rW = FT.band_fisher(S, Sa, P, pivot, r=r, X=p.X)
    gap = FT.metric(info, want)
    gm = _inf(info_mean - r * Rm) / _inf(r * Rm)
    print("%s (nt %d, W %d; the numpy factor fills W %d): %d probes, gap to the numpy sweep %.2e info_mean %.2e"
          % (name, nt, W, rW, nprobe, gap, gm))
    assert rW <= W and np.all(np.asarray(rhi) <= hi)
    assert gap <= FISHER_TOL
    assert gm <= 1e-10
    assert np.array_equal(info, info.T)


@pytest.mark.parametrize("name", ["flat9", "tall"])
def test_fisher_orthogonal_probes_equal_the_exact_mode(monkeypatch, name):
    """sqrt(n) Q, Q orthogonal, nprobe = n: sum_k e_k e_k' = n I, so the probe mode must give the exact mode's information
    (FISHER_TOL, info_mean to the bit: test_orthogonal_probes_equal_the_exact_mode)"""
    from scipy import linalg
    p = TE.problem(name)
    dirs = FT.standard_directions(3)
    Q = linalg.qr(np.random.default_rng(2 + p.n).standard_normal((p.n, p.n)))[0]
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        exact, em = fit.fisher_core(p.theta, dirs)
        got, gm = fit.fisher_core(p.theta, dirs, probes=np.sqrt(p.n) * Q)
    finally:
        fit.close()
    gap = FT.metric(got, exact)
    print("%s: %d orthogonal probes against the exact mode %.2e" % (name, p.n, gap))
    assert gap <= FISHER_TOL
    assert np.array_equal(gm, em)
