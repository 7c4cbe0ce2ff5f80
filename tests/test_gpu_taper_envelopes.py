"""Every entry of a tapered fit on band envelopes that are NOT flat -- wide in one place and at the floor in another (three
clusters among scattered sites), a clique laid out by the caller (columns eight tiles tall), a diagonal matrix, a chain, a
hub of stored zeros (W = nt - 1 packed, W = nt unpacked) and one stored zero far from the diagonal (the widest skew that
still packs) -- tests/taper_envelope_cases.py, seven named cases.

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
import taper_envelope_cases as TE  # noqa: E402
from test_gpu_cv_taper import BOUND as CV_BOUND  # noqa: E402
from test_gpu_fisher_taper import TOL as FISHER_TOL  # noqa: E402
from test_gpu_grad_taper import _fit_memory, _inf, _selinv  # noqa: E402
from test_gpu_krige_taper import ROUTE_TOL  # noqa: E402
from test_gpu_parity import N2LL_RTOL  # noqa: E402
from test_gpu_sim_taper import TOL as SIM_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

SL = TE.SMOOTH_LIMITS
ENTRIES = ["clusters", "clusters_caller", "hub", "hub_caller", "lshape", "islands"]
WITH_CHAIN = ENTRIES + ["chain"]
LAYOUTS = ["clusters", "hub", "lshape"]
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
    """(I at r = 1, X' S^-1 X) for the standard directions: tests/fisher_taper_reference.py"""
    from cocons_amd.host import theta_table
    p = TE.problem(base)
    S, Sa = FT.direction_matrices(theta_table(p.theta), p.locs, p.X, SL, p.ref_taper, FT.standard_directions(3))
    out = (FT.info_whiten(S, Sa, 1), FT.info_mean(S, p.X, 1))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_cv(base):
    """(e, var of cv_reference.cv_kroute for every observation; idx, e, var of cv_reference.cv_brute for every 8th (n > 1000)
    or 4th observation) on the dense S of grad_taper_reference, as test_gpu_cv_taper._reference.  Brute force is one Cholesky
    of order n - 1 per observation it predicts -- 19 s for the 1281 of clusters -- so it predicts a stride of them: each of
    these is a fold of its own, all the others share one fold whose result is dropped, and cv_brute's answer for a fold of
    one is the leave-one-out prediction whatever the other folds are.  The stride runs over the caller's order, which the
    handle's order scatters over every tile column.  Every observation is held to the route through the dense inverse, which
    test_leave_one_out_vs_reference uses above n = 700 and tests/test_cv_reference.py pins to brute force."""
    from cocons_amd.host import theta_table
    p = TE.problem(base)
    S, _ = GT.taper_matrix(theta_table(p.theta), p.locs, p.X, SL, p.ref_taper)
    S = np.tril(S) + np.tril(S, -1).T
    R = p.z - (p.X @ p.theta["mean"])[:, None]
    idx = np.arange(0, p.n, 8 if p.n > 1000 else 4)
    lab = np.full(p.n, -1)
    lab[idx] = idx
    eb, vb = CV.cv_brute(S, R, lab)
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
@pytest.mark.parametrize("name", WITH_CHAIN)
def test_value_and_parts(monkeypatch, name):
    """GetNeg2loglikelihoodTaper and its Profile form against the oracle (1e-8: test_taper_objective_vs_oracle); value and
    parts of neg2loglik_core against tests/grad_taper_reference.py (value 1e-9: test_value_and_gradient_vs_reference; every
    entry of parts 1e-9: tests/test_gpu_rhs_layouts.py); a second evaluation at a shifted theta on the same handle against the
    oracle (1e-8); then the first theta again: the first call's bits -- re-zeroing a varying envelope leaves no tile behind."""
    import cocons_amd as ca
    p = TE.problem(name)
    want, wantp, want2 = _ref_oracle_values(p.base)
    f, rparts = _ref_grad(p.base)[:2]
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
    R, Rm = _ref_fisher(p.base)
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


@pytest.mark.parametrize("name", ENTRIES)
def test_leave_one_out(monkeypatch, name):
    """cv_core against cv_reference.cv_brute at every 8th or 4th observation and against cv_reference.cv_kroute at every one
    (_ref_cv): gap_e and gap_v within 1e-8 (test_leave_one_out_vs_reference); two calls give the same bits."""
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
    be, bv = CV.gaps(got[0][where[idx]], got[1][where[idx]], eb, vb)
    re, rv = CV.gaps(e[idx], var[idx], eb, vb)
    print("%s: leave-one-out gap_e %.2e gap_v %.2e at all %d observations (dense inverse), %.2e %.2e at %d of them (brute "
          "force; the two references there: %.2e %.2e); var %.3g .. %.3g" % (name, ge, gv, p.n, be, bv, idx.size, re, rv,
                                                                          var.min(), var.max()))
    assert ge <= CV_BOUND and gv <= CV_BOUND
    assert be <= CV_BOUND and bv <= CV_BOUND
    assert _same(got, again)


@pytest.mark.parametrize("name", ENTRIES)
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


@pytest.mark.parametrize("name", WITH_CHAIN)
def test_held_factor_kriging(monkeypatch, name):
    """krige_taper_prepare(max_rows = 64), krige_taper_core on the 200 rows (four chunks, the last one of 8 rows): against
    predict_core on the same handle (4 x 1.912e-14 of the largest value: test_matches_the_one_shot_route; clusters_caller:
    1.656e-12, ten times the one-shot route's own distance from a long-double solve, see ROUTE_TOL_OF) and against the
    oracle (test_chunked_predict_vs_oracle); one chunk gives the same bits; so do the three whole 64-row blocks permuted.
    W = 6, 7 and 8 do not divide nt = 11 and 8: the ring wraps where no other test has it wrap."""
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


@pytest.mark.parametrize("name", ENTRIES)
def test_simulation(monkeypatch, name):
    """sim_core in the handle's own order with 65 draws (one more than a pass of band_trmm_kernel) against
    numpy.linalg.cholesky(S[order][:, order]) @ E + trend: 1e-10 of the largest value (test_fast_route_own_order).  clusters:
    also a pivot that is neither the handle's order nor the identity (test_draw_equal_route_pivot, the same bound)."""
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
        if name == "clusters":
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
    if name == "clusters":
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
    it at W = 5; here W = 6 and W = nt - 1).  COCONS_TAPER_BAND=0 (no envelope: another schedule) agrees in value (1e-12), parts
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
    import cocons_amd as ca
    p = TE.problem("clusters")
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
    f = _ref_grad("clusters")[0]
    print("clusters: value after two poisoned evaluations %.2e against the numpy statement" % (abs(first[0] - f) / abs(f)))
    assert abs(first[0] - f) <= 1e-9 * abs(f)
