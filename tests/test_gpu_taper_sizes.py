"""Every entry of a tapered fit at the sizes where the tile arithmetic degenerates -- one observation, two, one tile column
nearly empty and full (63 ... 128), two, three, four tile columns with and without a ragged last tile, and n = 640, the first
size whose band buffer packs (W = 4 of nt = 5) -- tests/taper_size_cases.py, fourteen sizes, p = 1 below three observations.

Every test first ASSERTS the shape from what the handle reports: nt and W of krige_taper_info() equal the restated rule
(taper_envelope_cases.envelope_of) on the order the handle reports and the size's row of the table, and
cocons_debug_fit_memory shows the unpacked buffer of nt + 1 tile rows at every size but 640, W + 1 there.  The entries --
value and parts, gradient, selected inverse, Fisher information exact and probed, leave-one-out, prediction, held-factor
kriging, joint prediction, simulation, failure and recovery -- are then held against the reference the suite has for each, at
the tolerance of the existing test of the same entry (imported where it is a constant, named at the comparison where it is a
literal there; none is loosened).  Every size runs in the library's own order; 128 and 640 also in the caller's.  Every test
prints its worst errors in one line that starts with `sizes-report` (tests/golden/SIZES_REPORT.md is made from them).
References are computed once per size."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
import fisher_taper_reference as FT  # noqa: E402
import grad_taper_reference as GT  # noqa: E402
import taper_envelope_cases as TE  # noqa: E402
import taper_size_cases as TS  # noqa: E402
from test_gpu_cv_taper import BOUND as CV_BOUND  # noqa: E402
from test_gpu_fisher_taper import TOL as FISHER_TOL  # noqa: E402
from test_gpu_grad_taper import _fit_memory, _inf, _selinv  # noqa: E402
from test_gpu_krige_taper import ROUTE_TOL, _err  # noqa: E402
from test_gpu_krige_taper_joint import TOL_COV, TOL_SIMS, TOL_STOCHASTIC, _dense, _eq  # noqa: E402
from test_gpu_parity import N2LL_RTOL  # noqa: E402
from test_gpu_sim_taper import TOL as SIM_TOL, _S, _want  # noqa: E402
from test_gpu_taper_envelopes import LAM, SL, _bad_thetas, _check_predict, _fit, _same  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, the library's own order?): every size in the library's order, 128 and 640 in the caller's too
CASES = [(n, True) for n in TS.TAPER_SIZES] + [(n, False) for n in TS.CALLER_ORDER_SIZES]
IDS = ["n%d" % n if rcm else "n%d_caller" % n for n, rcm in CASES]
sizes = pytest.mark.parametrize("n,rcm", CASES, ids=IDS)


def _report(entry, p, text):
    print("sizes-report taper | %s | %s | %s" % (entry, p.name, text))


# --------------------------------------------------------------------------- handles and their shape
def _assert_shape(fit, p, band=True):
    """The size's row of the table from what a FRESH handle reports (the rows under the matrix have not been regrown by a
    prediction): nt and W of krige_taper_info(), the leading dimension of the buffer.  Returns (order, nt, hi, W)."""
    order = fit.order()
    nt, hi, W, packed = TE.envelope_of(p.n, p.ref_taper[0], p.ref_taper[1], order)
    TS.assert_shape(p.n, nt, hi, W, packed, rcm=p.rcm)
    if not p.rcm:
        assert np.array_equal(order, np.arange(1, p.n + 1)), "the caller's order was not kept"
    info = fit.krige_taper_info()
    assert info["n"] == p.n and info["nt"] == nt, (info, nt)
    assert info["W"] == (W if band else nt), (info, W, hi.tolist())
    mem = _fit_memory(fit)
    if p.n == 640 and p.rcm and band and os.environ.get("COCONS_TAPER_PACKED") != "0":
        assert packed and W == 4 and mem[3] == (W + 1) * TE.TILE, mem
    else:
        assert mem[3] == (nt + 1) * TE.TILE, mem
    assert mem[0] == 8 * mem[3] * nt * TE.TILE, mem
    return order, nt, hi, W


def _theta_vector(th):
    """(optimiser vector with the mean free, par.pos) of a theta list of any number of columns"""
    from cocons_amd import workloads as wl
    cols = th["mean"].size
    pp = wl.par_pos_full(cols)
    pp["mean"] = [True] * cols
    return np.r_[th["mean"], wl.theta_vector_from_lists(th, wl.par_pos_full(cols))], pp


# --------------------------------------------------------------------------- references, once per size
@functools.lru_cache(maxsize=None)
def _ref_grad(n):
    """tests/grad_taper_reference.py at the size's theta: (f, parts, grad_logdet, grad_quad, grad_mean)"""
    from cocons_amd.host import theta_table
    p = TS.problem(n)
    out = GT.neg2loglik_taper_grad(theta_table(p.theta), p.theta["mean"], p.locs, p.X, p.z, SL, p.ref_taper)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_oracle_values(n):
    """the oracle's objective with the penalty, its Profile form (n > p), and the plain value at the shifted theta"""
    from oracle import oracle as O
    O.build()
    p = TS.problem(n)
    tv, pp = _theta_vector(p.theta)
    tv2, _ = _theta_vector(TS.shifted(p.theta))
    args = (p.ref_taper, p.locs, p.X, SL, p.z, p.n)
    prof = O.GetNeg2loglikelihoodTaperProfile(tv, pp, *args, LAM) if n > p.X.shape[1] else None
    return (O.GetNeg2loglikelihoodTaper(tv, pp, *args, LAM), prof, O.GetNeg2loglikelihoodTaper(tv2, pp, *args, (0.0, 0.0, 0.0)))


@functools.lru_cache(maxsize=None)
def _oracle_matrix(n):
    """S of the oracle on the size's pattern, in the caller's order (test_gpu_sim_taper._S)"""
    from oracle import oracle as O
    O.build()
    p = TS.problem(n)
    S = _S(O, p.theta, p.locs, p.X, p.ref_taper)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _ref_fisher(n):
    """(S, S_a, I at r = 1, X' S^-1 X) for the standard directions: tests/fisher_taper_reference.py"""
    from cocons_amd.host import theta_table
    p = TS.problem(n)
    S, Sa = FT.direction_matrices(theta_table(p.theta), p.locs, p.X, SL, p.ref_taper, FT.standard_directions(p.X.shape[1]))
    out = (S, Sa, FT.info_whiten(S, Sa, 1), FT.info_mean(S, p.X, 1))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_cv(n):
    """(e, var) of cv_reference.cv_brute and of cv_reference.cv_kroute at EVERY observation, on the dense S of
    grad_taper_reference (as test_gpu_cv_taper._reference): brute force is n factors of order n - 1, cheap at these sizes"""
    from cocons_amd.host import theta_table
    p = TS.problem(n)
    S, _ = GT.taper_matrix(theta_table(p.theta), p.locs, p.X, SL, p.ref_taper)
    S = np.tril(S) + np.tril(S, -1).T
    R = p.z - (p.X @ p.theta["mean"])[:, None]
    out = CV.cv_brute(S, R, np.arange(n)) + CV.cv_kroute(S, R, np.arange(n)) + (R, S[0, 0])
    for a in out[:5]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_predict(n):
    from oracle import oracle as O
    O.build()
    p = TS.problem(n)
    out = O.cocoPredict_sparse(p.theta, p.locs, p.lp, p.X, p.Xp, SL, p.z[:, 0], p.ref_taper, p.pred_taper)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_joint(n):
    """The dense numpy statement of test_gpu_krige_taper_joint._reference on the size's problem: (stochastic, S_uu, cov, mu);
    S_uu from the lower triangle of the uu pattern, mirrored."""
    from oracle import oracle as O
    O.build()
    p = TS.problem(n)
    uu = TS.uu_pattern(n)
    th, pt, m = p.theta, p.pred_taper, TS.M_PRED
    S = _dense(p.ref_taper, np.asarray(p.ref_taper[2]) * O.cov_rns_taper(th, p.locs, p.X, p.ref_taper[0], p.ref_taper[1], SL), n, n)
    C = _dense(pt, np.asarray(pt[2]) * O.cov_rns_taper_pred(th, p.locs, p.lp, p.X, p.Xp, pt[0], pt[1], SL), m, n)
    Su = np.tril(_dense(uu, np.asarray(uu[2]) * O.cov_rns_taper(th, p.lp, p.Xp, uu[0], uu[1], SL), m, m))
    Su = Su + np.tril(Su, -1).T
    SiCt = np.linalg.solve(S, C.T)
    st = (p.z[:, 0] - p.X @ th["mean"]) @ SiCt
    cov = Su - C @ SiCt
    out = (st, Su, (cov + cov.T) / 2, p.Xp @ th["mean"] + st)
    for a in out:
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------- entries
@sizes
def test_value_and_parts(monkeypatch, n, rcm):
    """GetNeg2loglikelihoodTaper and, for n > p, its Profile form against the oracle (N2LL_RTOL: test_taper_objective_vs_oracle);
    value and parts of neg2loglik_core against tests/grad_taper_reference.py (1e-9: test_value_and_gradient_vs_reference,
    tests/test_gpu_rhs_layouts.py); a shifted theta on the same handle against the oracle; then the first theta again: the
    first call's bits."""
    import cocons_amd as ca
    p = TS.problem(n, rcm)
    want, wantp, want2 = _ref_oracle_values(n)
    f, rparts = _ref_grad(n)[:2]
    tv, pp = _theta_vector(p.theta)
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        args = (p.ref_taper, p.locs, p.X, SL, p.z, p.n, LAM)
        got = ca.GetNeg2loglikelihoodTaper(tv, pp, *args, fit=fit)
        gotp = ca.GetNeg2loglikelihoodTaperProfile(tv, pp, *args, fit=fit) if wantp is not None else None
        v0 = fit.neg2loglik_core(p.theta)
        v2 = fit.neg2loglik_core(TS.shifted(p.theta))
        v1 = fit.neg2loglik_core(p.theta)
    finally:
        fit.close()
    assert (wantp is None) == (n <= p.X.shape[1]) == (n == 1)
    e = (abs(got - want) / abs(want), 0.0 if wantp is None else abs(gotp - wantp) / abs(wantp), abs(v0[0] - f) / abs(f),
         _inf(v0[1] / rparts - 1), abs(v2[0] - want2) / abs(want2))
    _report("value", p, "objective %.2e Profile %.2e value %.2e parts %.2e shifted theta %.2e" % e)
    assert e[0] <= N2LL_RTOL and e[1] <= N2LL_RTOL and e[4] <= N2LL_RTOL
    assert e[2] <= 1e-9 and e[3] <= 1e-9
    assert v1[0] == v0[0] and np.array_equal(v1[1], v0[1]), "the first theta again"
    assert v2[0] != v0[0]


@sizes
def test_gradient(monkeypatch, n, rcm):
    """neg2loglik_grad_core as test_gpu_taper_envelopes.test_gradient holds it: value and parts equal the value entry's (1e-12),
    grad_theta, grad_quad and grad_mean against the numpy statement (1e-7 of each one's largest component), value 1e-9, the
    scaling identity (1e-9 r n), two calls the same bits, the value call afterwards the bits it gave before."""
    p = TS.problem(n, rcm)
    f, rparts, rl, rq, rm = _ref_grad(n)
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
    assert gt.shape == gq.shape == rl.shape and gm.shape == rm.shape
    assert np.all(gt[2] == 0) and np.all(gt[3] == 0) and np.all(gq[2] == 0) and np.all(gq[3] == 0)
    errs = [_inf(g - w) / _inf(w) for g, w in ((gt, rl + rq), (gq, rq), (gm, rm))]
    ident = gt[0, 0] + gt[5, 0] - (r * p.n - float(np.sum(parts[1:])))
    _report("gradient", p, "value %.2e value entry %.2e parts %.2e grad_theta %.2e grad_quad %.2e grad_mean %.2e identity %.2e"
            % (abs(v - f) / abs(f), abs(v - v0) / abs(v0), _inf(parts - p0) / _inf(p0), errs[0], errs[1], errs[2],
               abs(ident) / (r * p.n)))
    assert abs(v - v0) <= 1e-12 * abs(v0)
    assert _inf(parts - p0) <= 1e-12 * _inf(p0)
    assert max(errs) <= 1e-7, errs
    assert abs(v - f) <= 1e-9 * abs(f)
    assert abs(ident) <= 1e-9 * r * p.n


@sizes
def test_selected_inverse(monkeypatch, n, rcm):
    """cocons_debug_taper_selinv at every stored entry against numpy.linalg.inv of the oracle's matrix: 1e-10 of max |S^-1|
    (test_selected_inverse_vs_dense_inverse); a repeated call gives the same bits.  nt = 1: only the triangular inverse and the
    diagonal kernel of launch_selinv run."""
    p = TS.problem(n, rcm)
    ci, rp, ent = p.ref_taper
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        got, _ = _selinv(fit, p.theta, ci.size)
        got2, _ = _selinv(fit, p.theta, ci.size)
    finally:
        fit.close()
    rows = np.repeat(np.arange(p.n), np.diff(rp))
    want = np.linalg.inv(_oracle_matrix(n))[rows, ci - 1]
    _report("selected inverse", p, "%.2e of max |S^-1| = %.3g over %d stored entries" % (_inf(got - want) / _inf(want), _inf(want),
                                                                                       ci.size))
    assert _inf(got - want) <= 1e-10 * _inf(want)
    assert np.array_equal(got, got2)


@sizes
def test_fisher_exact_mode(monkeypatch, n, rcm):
    """fisher_core, exact mode, standard_directions(p), in chunks of 64 probe rows and in the default's: the same bits; the gap
    to tests/fisher_taper_reference.py within FISHER_TOL and info_mean within 1e-10 (test_exact_mode_against_reference); both
    symmetric to the bit.  One and two tile columns: the backward sweep on the flipped factor at its shortest."""
    p = TS.problem(n, rcm)
    _, _, R, Rm = _ref_fisher(n)
    r = p.z.shape[1]
    dirs = FT.standard_directions(p.X.shape[1])
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        info, info_mean = fit.fisher_core(p.theta, dirs, max_rows=64)
        info0, info_mean0 = fit.fisher_core(p.theta, dirs, max_rows=0)
    finally:
        fit.close()
    gap = FT.metric(info, r * R)
    gm = _inf(info_mean - r * Rm) / _inf(r * Rm)
    _report("fisher exact", p, "gap %.2e info_mean %.2e I(v_s, v_s) - r n / 2 %.2e" % (gap, gm, info[-1, -1] - r * p.n / 2))
    assert info.shape == (dirs.shape[0],) * 2 and info_mean.shape == (p.X.shape[1],) * 2
    assert gap <= FISHER_TOL
    assert gm <= 1e-10
    assert np.array_equal(info, info.T) and np.array_equal(info_mean, info_mean.T)
    assert np.array_equal(info0, info) and np.array_equal(info_mean0, info_mean), "the chunk size changed the bits"


@sizes
@pytest.mark.parametrize("nprobe", [64, 100])
def test_fisher_probe_mode(monkeypatch, n, rcm, nprobe):
    """random +-1 probes through the handle's own order against the same probes through fisher_taper_reference.band_fisher with
    the handle's pivot: FISHER_TOL, info_mean 1e-10 (test_probe_mode_against_the_numpy_sweep); 100 probes leave the second
    strip partly filled"""
    p = TS.problem(n, rcm)
    S, Sa, _, Rm = _ref_fisher(n)
    r = p.z.shape[1]
    dirs = FT.standard_directions(p.X.shape[1])
    P = np.random.default_rng(nprobe + n).integers(0, 2, size=(n, nprobe)) * 2.0 - 1.0
    fit = _fit(monkeypatch, p)
    try:
        pivot = _assert_shape(fit, p)[0]
        info, info_mean = fit.fisher_core(p.theta, dirs, probes=P)
    finally:
        fit.close()
    want = FT.band_fisher(S, Sa, P, pivot, r=r, X=p.X)[0]
    gap = FT.metric(info, want)
    gm = _inf(info_mean - r * Rm) / _inf(r * Rm)
    _report("fisher %d probes" % nprobe, p, "gap to the numpy sweep %.2e info_mean %.2e" % (gap, gm))
    assert gap <= FISHER_TOL
    assert gm <= 1e-10
    assert np.array_equal(info, info.T)


@sizes
def test_leave_one_out(monkeypatch, n, rcm):
    """cv_core against cv_reference.cv_brute and cv_reference.cv_kroute at every observation: gap_e and gap_v within CV_BOUND
    (test_leave_one_out_vs_reference); two calls give the same bits.  n = 1: leaving the one observation out leaves nothing;
    the references give error = residual and variance = S_11, and so must the device."""
    p = TS.problem(n, rcm)
    eb, vb, ek, vk, R, s11 = _ref_cv(n)
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        got = fit.cv_core(p.theta)
        again = fit.cv_core(p.theta)
    finally:
        fit.close()
    assert got[0].shape == p.z.shape and got[1].shape == (p.n,)
    be, bv = CV.gaps(got[0], got[1], eb, vb)
    ke, kv = CV.gaps(got[0], got[1], ek, vk)
    _report("leave-one-out", p, "brute force gap_e %.2e gap_v %.2e dense inverse gap_e %.2e gap_v %.2e" % (be, bv, ke, kv))
    assert be <= CV_BOUND and bv <= CV_BOUND
    assert ke <= CV_BOUND and kv <= CV_BOUND
    if n == 1:
        assert np.array_equal(eb, R) and vb[0] == s11
        assert _inf(got[0] - R) <= CV_BOUND * np.sqrt(s11) and abs(got[1][0] - s11) <= CV_BOUND * s11
    assert _same(got, again)


@sizes
def test_prediction(monkeypatch, n, rcm):
    """predict_core against the oracle's cocoPredict_sparse at the bounds of _check_predict; the row without a neighbour gives
    exactly 0; the objective's bits are the same before and after."""
    p = TS.problem(n, rcm)
    want = _ref_predict(n)
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        v0 = fit.neg2loglik_core(p.theta)
        st, qf = fit.predict_core(p.theta, p.lp, p.Xp, p.pred_taper)
        v1 = fit.neg2loglik_core(p.theta)
    finally:
        fit.close()
    _report("prediction", p, "stochastic %.2e sd.pred %.2e" % _predict_errors(p, st, qf, want))
    _check_predict_at("predict_core", p, st, qf, want)
    assert qf[p.special[1]] == 0.0
    assert v1[0] == v0[0] and np.array_equal(v1[1], v0[1])


def _check_predict_at(tag, p, st, qf, want):
    """_check_predict of test_gpu_taper_envelopes on the size's prediction set.  Below three observations (the intercept alone)
    the predictive variance of the row on top of an observation is zero, the prediction there reproduces the observation and
    sd.pred is the square root of rounding error (tests/taper_size_cases.py): that row is held to what it must be instead --
    quadform equal to the site's variance within 64 ulp, the stochastic part at the bound of the others -- and _check_predict
    runs on the other 129 rows."""
    if p.n >= 3:
        return _check_predict(tag, p, st, qf, want)
    keep = np.delete(np.arange(TS.M_PRED), TS.ON_TOP)
    q = p._replace(Xp=p.Xp[keep], special=(None, int(np.nonzero(keep == TS.EMPTY)[0][0]), None))
    _check_predict(tag, q, st[keep], qf[keep], dict((k, v[keep]) for k, v in want.items()))
    var = float(np.exp(p.Xp[TS.ON_TOP] @ p.theta["std.dev"]) + np.exp(p.Xp[TS.ON_TOP] @ p.theta["nugget"]))
    resid = want["stochastic"][TS.ON_TOP]
    print("%s %s: on top of the observation: quadform - variance %.2e of it, stochastic %.2e"
          % (p.name, tag, (qf[TS.ON_TOP] - var) / var, abs(st[TS.ON_TOP] - resid) / abs(resid)))
    assert abs(qf[TS.ON_TOP] - var) <= 64 * np.finfo(float).eps * var
    assert abs(st[TS.ON_TOP] - resid) < 1e-10 * _inf(want["stochastic"])


def _predict_errors(p, st, qf, want):
    """(stochastic, sd.pred) as _check_predict measures them; below three observations without the row on top of an
    observation (_check_predict_at)"""
    from cocons_amd.host import _sparse_predict_tail
    got = _sparse_predict_tail(p.theta, p.Xp, st, qf, "pred")
    rows = np.arange(TS.M_PRED) if p.n >= 3 else np.delete(np.arange(TS.M_PRED), TS.ON_TOP)
    return (_inf((got["stochastic"] - want["stochastic"])[rows]) / _inf(want["stochastic"][rows]),
            _inf((got["sd.pred"] - want["sd.pred"])[rows]) / _inf(want["sd.pred"][rows]))


@sizes
def test_held_factor_kriging(monkeypatch, n, rcm):
    """krige_taper_prepare(max_rows = 64), krige_taper_core on the 130 rows (chunks of 64, 64 and 2): against predict_core on
    the same handle (ROUTE_TOL: test_matches_the_one_shot_route) and against the oracle (_check_predict); max_rows = 256 (one
    chunk) gives the same bits; the first row alone, the first 64 rows and rows 64 ... 129 each give the bits of those rows in
    the full call.  W = nt = 1: a ring of one slot."""
    p = TS.problem(n, rcm)
    want = _ref_predict(n)
    fit = _fit(monkeypatch, p)
    try:
        order, nt, hi, W = _assert_shape(fit, p)
        one_shot = fit.predict_core(p.theta, p.lp, p.Xp, p.pred_taper)
        fit.krige_taper_prepare(p.theta, max_rows=64)
        info = fit.krige_taper_info()
        assert info["prepared"] and info["rows"] == 64 and info["W"] == W and info["nt"] == nt
        got = fit.krige_taper_core(p.lp, p.Xp, p.pred_taper)
        parts = []
        for idx in (np.arange(1), np.arange(64), np.arange(64, TS.M_PRED)):
            parts.append((idx, fit.krige_taper_core(p.lp[idx], p.Xp[idx], TS.take_rows(p.pred_taper, idx))))
        fit.krige_taper_prepare(p.theta, max_rows=256)
        assert fit.krige_taper_info()["rows"] == 256
        whole = fit.krige_taper_core(p.lp, p.Xp, p.pred_taper)
    finally:
        fit.close()
    e = _err(got, one_shot)
    _report("held-factor kriging", p, "against the one-shot route stochastic %.3e quadform %.3e; oracle stochastic %.2e sd.pred %.2e"
            % (e + _predict_errors(p, got[0], got[1], want)))
    _check_predict_at("krige_taper_core", p, got[0], got[1], want)
    assert max(e) <= ROUTE_TOL, e
    assert got[0][p.special[1]] == 0.0 and got[1][p.special[1]] == 0.0
    assert _same(whole, got), "one chunk"
    for idx, sub in parts:
        assert sub[0].shape == (idx.size,)
        assert np.array_equal(sub[0], got[0][idx]) and np.array_equal(sub[1], got[1][idx]), "rows %d ... %d alone" % (idx[0], idx[-1])


@sizes
def test_joint_prediction(monkeypatch, n, rcm):
    """krige_taper_joint against the dense numpy statement of test_gpu_krige_taper_joint._reference at that file's bounds
    (TOL_COV, TOL_SIMS, TOL_STOCHASTIC; above 1e-10 a defect): the covariance on the 130 rows, and covariance and three draws
    on the 129 rows off the observation (with the row on top of an observation the predictive covariance is singular or
    indefinite, tests/taper_size_cases.py: no draw is defined there).  The stochastic part has the bits of apply; the covariance
    is symmetric to the bit; depths 1, 2 and the default give the same bits (at nt <= 2 every depth hits the
    min(W + depth - 1, nt) clamp of the ring); the first row alone gives the [0, 0] entry of the full covariance to the bit
    (test_bit_exactness claims it for leading blocks), and its draws are held to the reference too."""
    p = TS.problem(n, rcm)
    uu = TS.uu_pattern(n)
    st_ref, Su, cov_ref, mu = _ref_joint(n)
    rows = TS.draw_rows()
    sub_ref = cov_ref[np.ix_(rows, rows)]
    ev = np.linalg.eigvalsh(sub_ref)
    assert ev.min() > 0
    E = np.random.default_rng(70 + n).standard_normal((TS.M_PRED, 3))
    monkeypatch.delenv("COCONS_KRIGE_JOINT_DEPTH", raising=False)
    fit = _fit(monkeypatch, p)
    try:
        _assert_shape(fit, p)
        fit.krige_taper_prepare(p.theta)
        st0, qf0 = fit.krige_taper_core(p.lp, p.Xp, p.pred_taper)
        st, cov, none = fit.krige_taper_joint_core(p.lp, p.Xp, p.pred_taper, uu)
        sub = (p.lp[rows], p.Xp[rows], TS.take_rows(p.pred_taper, rows), TS.sub_pattern(uu, rows))
        drawn = fit.krige_taper_joint_core(*sub, iiderrors=E[rows])
        again = (fit.krige_taper_joint_core(p.lp, p.Xp, p.pred_taper, uu), fit.krige_taper_joint_core(*sub, iiderrors=E[rows]))
        depths = {}
        for depth in ("1", "2"):
            monkeypatch.setenv("COCONS_KRIGE_JOINT_DEPTH", depth)
            depths[depth] = (fit.krige_taper_joint_core(p.lp, p.Xp, p.pred_taper, uu),
                             fit.krige_taper_joint_core(*sub, iiderrors=E[rows]))
        monkeypatch.delenv("COCONS_KRIGE_JOINT_DEPTH")
        first = fit.krige_taper_joint_core(p.lp[:1], p.Xp[:1], TS.take_rows(p.pred_taper, np.arange(1)),
                                           TS.sub_pattern(uu, np.arange(1)), iiderrors=E[:1])
    finally:
        fit.close()
    assert none is None
    top = float(np.max(np.diag(cov_ref)))
    want = np.linalg.cholesky(sub_ref) @ E[rows] + mu[rows, None]
    e_cov = _inf(cov - cov_ref) / top
    e_sub = _inf(drawn[1] - sub_ref) / float(np.max(np.diag(sub_ref)))
    e_sims = _inf(drawn[2] - want) / _inf(want)
    e_st = _inf(st - st_ref) / _inf(st_ref)
    e_qf = _inf((np.diag(Su) - np.diag(cov)) - qf0) / top
    want1 = np.sqrt(cov_ref[0, 0]) * E[0] + mu[0]
    e_one = _inf(first[2][0] - want1) / _inf(want1)
    _report("joint prediction", p, "cov %.3e (129 rows %.3e) sims %.3e stochastic %.3e diag against quadform %.3e first row's "
            "draws %.3e (eigenvalues %.3e .. %.3e)" % (e_cov, e_sub, e_sims, e_st, e_qf, e_one, ev.min(), ev.max()))
    assert np.array_equal(st, st0), "the stochastic part is apply's"
    assert np.array_equal(drawn[0], st0[rows])
    assert np.array_equal(cov, cov.T) and np.array_equal(drawn[1], drawn[1].T)
    assert _eq(again[0], (st, cov, None)) and _eq(again[1], drawn)
    for depth, (b, d) in depths.items():
        assert _eq(b, (st, cov, None)) and _eq(d, drawn), "depth " + depth
    assert st[p.special[1]] == 0.0 and np.count_nonzero(cov[p.special[1]]) == 1 and cov[p.special[1], p.special[1]] > 0
    assert first[1].shape == (1, 1) and first[1][0, 0] == cov[0, 0] and first[0][0] == st[0]
    assert max(e_cov, e_sub, e_sims, e_st, e_one) <= 1e-10, "a defect, not a bound"
    assert e_cov <= TOL_COV and e_sub <= TOL_COV and e_sims <= TOL_SIMS and e_st <= TOL_STOCHASTIC, (e_cov, e_sub, e_sims, e_st)
    assert e_qf <= TOL_COV and e_one <= TOL_SIMS, (e_qf, e_one)


@sizes
def test_simulation(monkeypatch, n, rcm):
    """sim_core in the handle's own order with 65 draws (one more than a pass of band_trmm_kernel) against
    numpy.linalg.cholesky(S[order][:, order]) @ E + trend at SIM_TOL (test_fast_route_own_order); n = 128 and 640: also a pivot
    that is neither the handle's order nor the identity (test_draw_equal_route_pivot, the same bound); a repeated call gives the
    same bits."""
    p = TS.problem(n, rcm)
    S = _oracle_matrix(n)
    rng = np.random.default_rng(65 + p.n)
    E = rng.standard_normal((p.n, 65))
    trend = p.X @ p.theta["mean"]
    with_pivot = n in (128, 640)
    fit = _fit(monkeypatch, p)
    try:
        order = _assert_shape(fit, p)[0]
        got = fit.sim_core(p.theta, E)
        again = fit.sim_core(p.theta, E)
        if with_pivot:
            piv = (rng.permutation(p.n) + 1).astype(np.int32)
            assert not np.array_equal(piv, order) and not np.array_equal(piv, np.arange(1, p.n + 1))
            got_piv = fit.sim_core(p.theta, E, pivot=piv)
            own_after = fit.sim_core(p.theta, E)
    finally:
        fit.close()
    want = _want(S, order, E, trend)
    e = _inf(got - want) / _inf(want)
    e_piv = 0.0
    assert got.shape == (p.n, 65) and e <= SIM_TOL, e
    assert np.array_equal(got, again)
    if with_pivot:
        want_piv = _want(S, piv, E, trend)
        e_piv = _inf(got_piv - want_piv) / _inf(want_piv)
    _report("simulation", p, "65 draws in the handle's order %.2e, with a caller's pivot %.2e" % (e, e_piv))
    if with_pivot:
        assert e_piv <= SIM_TOL, e_piv
        assert np.array_equal(own_after, got) and not np.array_equal(got_piv, got)


# --------------------------------------------------------------------------- failure and recovery
@pytest.mark.parametrize("n", [1, 128, 257])
def test_failure_and_recovery(monkeypatch, n):
    """A NaN theta and a theta whose matrix is not positive definite (_bad_thetas) each poison every tile the factorisation
    touches -- one tile, a full tile, three tile columns with a ragged last one; the first theta afterwards gives the first
    call's bits, value and gradient (test_recovery_on_a_wide_envelope)."""
    import cocons_amd as ca
    p = TS.problem(n)
    nan, npd = _bad_thetas(p.theta)
    tv, pp = _theta_vector(p.theta)
    tv_nan = tv.copy()
    tv_nan[p.X.shape[1]] = np.nan                                  # the first parameter behind the mean
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
    f = _ref_grad(n)[0]
    _report("recovery", p, "value after the poisoned evaluations %.2e against the numpy statement" % (abs(first[0] - f) / abs(f)))
    assert abs(first[0] - f) <= 1e-9 * abs(f)


# --------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("n", [128, 640])
def test_buffer_layouts(monkeypatch, n):
    """COCONS_TAPER_PACKED=0 and COCONS_TAPER_BAND=0 held to the default as in test_gpu_taper_envelopes.test_buffer_layouts.
    n = 640: the packed default (W + 1 = 5 tile rows) against the dense buffer with its band used (the same schedule: the same
    bits) and against no envelope (another schedule: value and parts 1e-12, gradient 1e-10 of the largest component of
    grad_theta).  n = 128: one tile column, nothing to pack -- all three are the SAME layout (leading dimension 2 x 128); the
    first two are the same handle and give the same bits, the third keeps the bounds of the other schedule."""
    p = TS.problem(n)
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
    if n == 640:
        assert lda["packed"] == (W + 1) * TE.TILE < lda["unpacked"] == lda["noband"] == (nt + 1) * TE.TILE, lda
    else:
        assert lda["packed"] == lda["unpacked"] == lda["noband"] == (nt + 1) * TE.TILE == 2 * TE.TILE, lda
    a, b, c = res["packed"], res["unpacked"], res["noband"]
    assert len(a) == len(b) == 13
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "output %d differs between the packed and the dense buffer" % k
    assert a[11] == a[0] and np.array_equal(a[12], a[1])
    e_v, e_p = abs(c[0] - a[0]) / abs(a[0]), _inf(c[1] - a[1]) / _inf(a[1])
    e_g = [_inf(c[k] - a[k]) / _inf(a[4]) for k in (4, 5, 6)]
    _report("buffer layouts", p, "no envelope against the default: value %.2e parts %.2e gradient %.2e %.2e %.2e"
            % ((e_v, e_p) + tuple(e_g)))
    assert e_v <= 1e-12 and e_p <= 1e-12
    assert max(e_g) <= 1e-10
