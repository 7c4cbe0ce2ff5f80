"""Every layout the right-hand sides of an evaluation can take through the factorisation -- slot rows inside the matrix's last
tile (16 to 112 of them, partly and exactly full), one or two tile rows under the matrix with and without the trimmed last 64
rows, front padding together with a border, a handle whose dense and Profile calls fall on opposite sides of a boundary, the
gradients' wider leading dimension (r + nxb > 128), krige / predict with a far z_col -- with many realisations (r up to 190)
and wide designs (p = q = 32), on every schedule that exists at the size: plain (up to 4 tiles), classic engine and
dependency-driven (5 tiles and more).

Every case ASSERTS the layout it claims through cocons_debug_rhs_layout (the function the evaluation itself asks), so a change
of the layout rule makes these tests say so.  Values, parts and GLS coefficients are held against tests/rhs_layout_reference.py
(long-double Cholesky, long-double Gram matrix; pinned to the R closures' restatements by tests/test_rhs_layout_reference.py)
at the tolerances the suite already holds against oracle.chol_ld: 1e-9 relative for the value and every entry of parts, 1e-9
of the largest coefficient for the GLS coefficients.  Each test prints its worst relative errors."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict, namedtuple

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rhs_layout_reference as RL  # noqa: E402
from test_gpu_grad import _zero_matrix_theta  # noqa: E402

pytestmark = pytest.mark.gpu

SL = (0.5, 2.5)                      # workloads.SMOOTH_LIMITS

# (slots, tile rows under the matrix, trim) of the dense (r rows), Profile (r + q) and REML (r + p) operations; q = p
Case = namedtuple("Case", "name n p r pad0 nslot dense wide")
SLOTS = (1, 0, 0)
CASES = [
    Case("L1", 700, 3, 13, 52, 16, SLOTS, SLOTS),              # 16 slots: 13 in use, then exactly full
    Case("L2", 700, 3, 61, 4, 64, SLOTS, SLOTS),               # 64 slots, exactly full with Profile
    Case("L3", 700, 3, 62, 68, 0, (0, 1, 1), (0, 1, 0)),       # need 80 > 68: border; 62 rows trimmed, 65 not
    Case("L4", 768, 3, 64, 0, 0, (0, 1, 1), (0, 1, 0)),        # exactly 64 rows: still trimmed; 67: not
    Case("L5", 768, 3, 126, 0, 0, (0, 1, 0), (0, 2, 1)),       # 126: one tile row; 129: two, the second trimmed
    Case("L6", 768, 3, 190, 0, 0, (0, 2, 1), (0, 2, 0)),       # two tile rows, 190 trimmed, 193 not
    Case("L7", 640, 3, 65, 0, 0, (0, 1, 0), (0, 1, 0)),        # five tiles (a last block of one tile), untrimmed
    Case("L8", 641, 3, 109, 15, 112, SLOTS, SLOTS),            # the last tile holds 16 observations and 112 slots
    Case("L9", 700, 32, 3, 20, 48, SLOTS, SLOTS),              # wide design: 35 of 48 slots
    Case("L10", 768, 32, 40, 0, 0, (0, 1, 1), (0, 1, 0)),      # wide design: 72 rows, untrimmed
    Case("L11", 300, 3, 61, 20, 64, SLOTS, SLOTS),             # plain schedule, 64 slots
    Case("L12", 384, 3, 126, 0, 0, (0, 1, 0), (0, 2, 1)),      # plain schedule, two tile rows
    Case("L13", 500, 3, 13, 12, 0, (0, 1, 1), (0, 1, 1)),      # need 16 > 12: front padding AND a border
    Case("L14a", 1, 1, 20, 95, 32, SLOTS, SLOTS),              # one observation, 20 realisations
    Case("L14b", 65, 1, 130, 63, 0, (0, 2, 1), (0, 2, 1)),     # 65 observations, 130 realisations
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
SCHEDULED = [c.name for c in CASES if c.n >= 640]
FULL = ["L1", "L2", "L8", "L11"]           # Profile / REML fill the slots exactly
KRIGED = ["L2", "L5", "L8"]
GRADIENTS = ["L2", "L3", "L5", "L8", "L9"]


def _seed(c):
    return 9000 + 10 * c.n + c.r + c.p


@functools.lru_cache(maxsize=None)
def _problem_cached(name):
    c = BY_NAME[name]
    out = RL.layout_problem(c.n, c.p, c.r, _seed(c))
    for a in out[:2] + out[3:]:
        a.setflags(write=False)
    return out


def _problem(c):
    return _problem_cached(c.name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(dense, profile, reml) = (value, parts) each, computed once per case and shared by its tests.  Profile and REML read
    the same Gram matrix (x_betas = X)."""
    from oracle import oracle as O
    O.build()
    c = BY_NAME[name]
    locs, X, th, z = _problem(c)
    # one observation and an intercept: z' P z = 0 exactly, the reference's cancellation bound cannot hold (see _compare)
    check = c.n > c.p
    d = RL.dense(O, th, locs, X, z, SL)
    ld_gram = RL.gram(O, th, locs, X, np.column_stack([z, X]), SL)
    pr = RL.profile(O, th, locs, X, z, X, SL, check=check, ld_gram=ld_gram)
    rm = RL.profile(O, th, locs, X, z, X, SL, reml=True, check=check, ld_gram=ld_gram)
    print("%s reference: cond(W) %.1f, max g' W^-1 g / G_kk %.3f" % (name, pr[2]["cond_W"], pr[2]["ratio"]))
    for a in (d[1], pr[1], rm[1]):
        a.setflags(write=False)
    return d, pr[:2], rm[:2]


def _fit(c):
    import cocons_amd as ca
    locs, X, th, z = _problem(c)
    return ca.CoconsFit(locs, X, z, SL, x_betas=X)


def _layout(fit, nxb):
    out = (ctypes.c_int * 5)()
    assert fit._L.cocons_debug_rhs_layout(fit._h, int(nxb), out) == 0
    return list(out)


def _assert_layout(fit, c):
    """the case's row of the table, from the function the evaluations themselves ask"""
    assert _layout(fit, 0) == [c.pad0, c.nslot] + list(c.dense), (c.name, _layout(fit, 0))
    assert _layout(fit, c.p) == [c.pad0, c.nslot] + list(c.wide), (c.name, _layout(fit, c.p))
    if c.name in FULL:
        assert c.r + c.p == c.nslot


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(a - b) / np.abs(b)
    e = np.where(a == b, 0.0, e)
    return float(np.max(e)) if e.size else 0.0


def _compare(label, c, got, want, nxb):
    """value 1e-9 relative; parts[0 .. 1 + r] (log-determinants, quadratic forms) each 1e-9 relative; GLS coefficients 1e-9 of
    the largest one (test_profile_betas_vs_numpy).  n <= p (L14a: one observation, an intercept): the Profile / REML quadratic
    forms are G_kk - g_k^2 / W = 0 exactly, so they are held to 1e-9 of the G_kk they cancel from (double rounding of the
    three Gram entries gives a few 1e-16 G_kk) instead of a relative error of zero; and the REML value there is
    sum_k 2 ld + 2 ldW + 0 with W = 1 / Sigma, zero as well, so it is held to 1e-9 of the terms it is summed from."""
    v, parts = got
    rv, rparts = want
    r = c.r
    head = 2 if nxb else 1
    assert parts.shape == rparts.shape == (head + r + nxb,)
    scale_v = abs(rv)
    if nxb and c.n <= c.p:
        scale_v = r * (c.n * np.log(2 * np.pi) + 2 * float(np.sum(np.abs(rparts[:head]))))
    e_v = abs(v - rv) / scale_v
    e_ld = _rel(parts[:head], rparts[:head])
    quad, rquad = parts[head:head + r], rparts[head:head + r]
    if nxb and c.n <= c.p:
        from oracle import oracle as O
        locs, X, th, z = _problem(c)
        gkk = z[0] ** 2 / float(O.cov_rns(th, locs, X, SL)[0, 0])                       # n = p = 1: Sigma is 1 x 1
        e_q = float(np.max(np.abs(quad - rquad) / gkk))
    else:
        e_q = _rel(quad, rquad)
    e_b = float(np.max(np.abs(parts[head + r:] - rparts[head + r:])) / np.max(np.abs(rparts[head + r:]))) if nxb else 0.0
    print("%s %-22s value %.2e  logdets %.2e  quadratic forms %.2e  betas %.2e" % (c.name, label, e_v, e_ld, e_q, e_b))
    assert e_v <= 1e-9, (label, e_v)
    assert e_ld <= 1e-9, (label, e_ld)
    assert e_q <= 1e-9, (label, e_q)
    assert e_b <= 1e-9, (label, e_b)


def _three(fit, c, th):
    rank = int(np.linalg.matrix_rank(_problem(c)[1]))
    return fit.neg2loglik_core(th), fit.neg2loglik_profile_core(th), fit.neg2loglik_reml_core(th, rank)


def _same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


def _tune(name, value):
    from cocons_amd import _lib
    _lib.check(_lib.load().cocons_debug_tune(name.encode(), int(value)), "cocons_debug_tune")


@pytest.fixture
def schedules():
    """yields a function that selects a schedule; the process's own settings come back afterwards"""
    def select(which):
        _tune("engine", 0 if which == "plain" else 1)
        _tune("dag", 1 if which == "dag" else 0)
        _tune("dag_min_tiles", 0)
    yield select
    _tune("engine", int(os.environ.get("COCONS_ENGINE", "1")))
    _tune("dag", int(os.environ.get("COCONS_DAG", "1")))
    _tune("dag_min_tiles", int(os.environ.get("COCONS_DAG_MIN_TILES", "2000")))


def _dag_steps(fit):
    """steps of the persistent launch the handle's last engine start prepared (0: none)"""
    ns = ctypes.c_int(0)
    rc = fit._L.cocons_debug_dag_trace(fit._h, ctypes.byref(ns), None, None, None)
    return ns.value if rc >= 0 else 0


@pytest.mark.parametrize("name", IDS)
def test_values_bits_recovery_and_batch(oracle, name):
    """(a) dense, Profile and REML against the reference; (b) the dense call after them gives the first dense call's bits;
    (c) a failing evaluation in between (Sigma = 0: minor 1) leaves the next Profile call's bits alone; (e) the batch entry
    with 5 perturbed points equals the single calls to 1e-12."""
    import cocons_amd as ca
    c = BY_NAME[name]
    locs, X, th, z = _problem(c)
    ref = _reference(name)
    fit = _fit(c)
    try:
        _assert_layout(fit, c)
        d0, p0, r0 = _three(fit, c, th)
        d1 = fit.neg2loglik_core(th)
        for label, got, want, nxb in (("dense", d0, ref[0], 0), ("Profile", p0, ref[1], c.p), ("REML", r0, ref[2], c.p)):
            _compare(label, c, got, want, nxb)
        assert _same_bits(d1, d0), "dense call after Profile / REML"
        with pytest.raises(ca.CholeskyError) as ei:
            fit.neg2loglik_profile_core(_zero_matrix_theta(th))
        assert ei.value.minor == 1
        p1 = fit.neg2loglik_profile_core(th)
        assert _same_bits(p1, p0), "Profile call after a failing evaluation"
        with pytest.raises(ca.CholeskyError) as ei:
            fit.neg2loglik_core(_zero_matrix_theta(th))
        assert ei.value.minor == 1
        assert _same_bits(fit.neg2loglik_reml_core(th, int(np.linalg.matrix_rank(X))), r0)
        assert _same_bits(fit.neg2loglik_core(th), d0)
        pts = []
        for i in range(5):
            t = OrderedDict((k, np.array(v, float)) for k, v in th.items())
            t["scale"][0] += 0.03 * (i - 2)
            t["std.dev"][0] -= 0.02 * i
            t["mean"][0] += 0.01 * i
            pts.append(t)
        vals, st = fit.neg2loglik_batch_core(pts)
        one = np.array([fit.neg2loglik_core(t)[0] for t in pts])
        print("%s batch against single calls %.2e" % (name, _rel(vals, one)))
        assert np.all(st == 0)
        assert np.allclose(vals, one, rtol=1e-12, atol=0)
        assert _same_bits(fit.neg2loglik_core(th), d0)
        assert fit.engine_state()["retries"] == 0
    finally:
        fit.close()


@pytest.mark.skipif(os.environ.get("COCONS_ENGINE", "1") == "0", reason="COCONS_ENGINE=0: no engine schedules to compare")
@pytest.mark.parametrize("name", SCHEDULED)
def test_schedules_agree(oracle, schedules, name):
    """(d) five tiles and more: the three objectives under the dependency-driven schedule forced for every step, the classic
    engine schedule and the plain schedule -- each against the reference, against each other (values 1e-11, parts 1e-9 as
    test_dag_vs_classic_and_oracle), no hand-off time-out, and the schedule meant really ran."""
    c = BY_NAME[name]
    locs, X, th, z = _problem(c)
    ref = _reference(name)
    fit = _fit(c)
    got = {}
    try:
        _assert_layout(fit, c)
        for which in ("dag", "classic", "plain"):
            schedules(which)
            res = []
            rank = int(np.linalg.matrix_rank(X))
            for call in (lambda: fit.neg2loglik_core(th), lambda: fit.neg2loglik_profile_core(th),
                         lambda: fit.neg2loglik_reml_core(th, rank)):
                res.append(call())
                st = fit.engine_state()
                assert st["retries"] == 0, (which, st)
                assert st["active"] == (which != "plain"), (which, st)
                if which == "dag":
                    assert _dag_steps(fit) >= 2, "the dependency-driven schedule did not take this factorisation"
            assert _same_bits(fit.neg2loglik_core(th), res[0]), which
            got[which] = res
            for label, g, want, nxb in (("dense", res[0], ref[0], 0), ("Profile", res[1], ref[1], c.p), ("REML", res[2], ref[2], c.p)):
                _compare("%s / %s" % (label, which), c, g, want, nxb)
        for other in ("classic", "plain"):
            for k, label in enumerate(("dense", "Profile", "REML")):
                a, b = got["dag"][k], got[other][k]
                head = (2 if k else 1) + c.r
                print("%s %s dag against %s: value %.2e parts %.2e" % (name, label, other, abs(a[0] - b[0]) / abs(b[0]),
                                                                      _rel(a[1][:head], b[1][:head])))
                assert abs(a[0] - b[0]) <= 1e-11 * abs(b[0]), (label, other)
                assert np.allclose(a[1][:head], b[1][:head], rtol=1e-9, atol=0), (label, other)
                if k:
                    assert np.max(np.abs(a[1][head:] - b[1][head:])) <= 1e-9 * np.max(np.abs(b[1][head:])), (label, other)
    finally:
        fit.close()


@pytest.mark.parametrize("name", KRIGED)
def test_predict_and_krige_with_the_last_realisation(oracle, name):
    """predict_core with z_col = r - 1 and krige_core after a prepare with z_col = r - 1 at 70 new locations, on handles with 64
    and 112 slots and without any: against numpy.linalg.solve on the oracle's matrices (the tolerances of
    test_ragged_sizes_all_entry_points) and against each other (test_krige_matches_predict_core); the objective's bits
    survive both."""
    c = BY_NAME[name]
    locs, X, th, z = _problem(c)
    m = 70
    rng = np.random.default_rng(_seed(c) + 5)
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = np.column_stack([np.ones(m)] + [rng.standard_normal(m) * 0.3 for _ in range(c.p - 1)])
    S = oracle.cov_rns(th, locs, X, SL)
    Cw = oracle.cov_rns_pred(th, locs, lp, X, Xp, SL)
    sol = np.linalg.solve(S, Cw.T)
    want_st = (z[:, c.r - 1] - X @ th["mean"]) @ sol
    want_qf = np.sum(Cw * sol.T, axis=1)
    fit = _fit(c)
    try:
        _assert_layout(fit, c)
        d0 = fit.neg2loglik_core(th)
        st, qf = fit.predict_core(th, lp, Xp, z_col=c.r - 1)
        fit.krige_prepare(th, z_col=c.r - 1)
        kst, kqf = fit.krige_core(lp, Xp)
        d1 = fit.neg2loglik_core(th)
        kst2, kqf2 = fit.krige_core(lp, Xp)
    finally:
        fit.close()
    print("%s predict: stochastic %.2e quadform %.2e; krige against predict: %.2e %.2e"
          % (name, np.max(np.abs(st - want_st)) / np.max(np.abs(want_st)), _rel(qf, want_qf),
             np.max(np.abs(kst - st)) / np.max(np.abs(st)), _rel(kqf, qf)))
    assert np.allclose(st, want_st, rtol=1e-8, atol=1e-10)
    assert np.allclose(qf, want_qf, rtol=1e-8, atol=1e-12)
    assert np.allclose(kst, want_st, rtol=1e-8, atol=1e-10)
    assert np.allclose(kqf, want_qf, rtol=1e-8, atol=1e-12)
    assert np.max(np.abs(kst - st)) <= 1e-12 * np.max(np.abs(st))
    assert np.max(np.abs(kqf - qf) / np.abs(qf)) <= 1e-12
    assert _same_bits(d1, d0)
    assert np.array_equal(kst2, kst) and np.array_equal(kqf2, kqf)
    # the last realisation is not the first one: a z_col that is ignored would pass none of the above
    assert np.max(np.abs((z[:, 0] - X @ th["mean"]) @ sol - want_st)) > 1e-3 * np.max(np.abs(want_st))


@pytest.mark.parametrize("obj", ["dense", "pml", "reml"])
@pytest.mark.parametrize("name", GRADIENTS)
def test_gradients(name, obj):
    """The analytic gradients with many right-hand sides (L5: r + nxb = 129 > 128, the wider leading dimension; L9: p = 32)
    against tests/grad_reference.py and tests/grad_profile_reference.py at the tolerances of test_shapes_against_reference
    (value 1e-10, gradient 1e-7 of its largest entry); a second call gives the same bits; the value call afterwards gives
    the bits it gave before."""
    import grad_profile_reference as GPR
    import grad_reference as GR
    from cocons_amd.host import theta_table
    c = BY_NAME[name]
    locs, X, th, z = _problem(c)
    rank = int(np.linalg.matrix_rank(X))
    fit = _fit(c)
    try:
        _assert_layout(fit, c)
        if obj == "dense":
            value, grad = (lambda: fit.neg2loglik_core(th)), (lambda: fit.neg2loglik_grad_core(th))
        elif obj == "pml":
            value, grad = (lambda: fit.neg2loglik_profile_core(th)), (lambda: fit.neg2loglik_profile_grad_core(th))
        else:
            value, grad = (lambda: fit.neg2loglik_reml_core(th, rank)), (lambda: fit.neg2loglik_reml_grad_core(th, rank))
        v0 = value()
        g0 = grad()
        g1 = grad()
        v1 = value()
    finally:
        fit.close()
    assert _same_bits(v1, v0), "value call after the gradient calls"
    assert g1[0] == g0[0] and all(np.array_equal(a, b) for a, b in zip(g0[1:], g1[1:])), "second gradient call"
    assert abs(g0[0] - v0[0]) <= 1e-12 * abs(v0[0])
    if obj == "dense":
        f, rgt, rgm = GR.neg2loglik_grad(theta_table(th), th["mean"], locs, X, z, SL)
        g, rg = np.concatenate([g0[2].ravel(), g0[3]]), np.concatenate([rgt.ravel(), rgm])
    elif obj == "pml":
        f, rg, _, _ = GPR.profile_grad(th, locs, X, z, X, SL)
        g = g0[2]
    else:
        f, rg, _, _ = GPR.reml_grad(th, locs, X, z, SL)
        g = g0[2]
    e_v, e_g = abs(g0[0] - f) / abs(f), float(np.max(np.abs(g - rg)) / np.max(np.abs(rg)))
    print("%s %s gradient: value %.2e gradient %.2e of its largest entry" % (name, obj, e_v, e_g))
    assert e_v <= 1e-10
    assert e_g <= 1e-7


@pytest.mark.parametrize("r,trim", [(20, 1), (70, 0)])
def test_taper_handle_with_many_realisations(oracle, r, trim):
    """A taper handle (caller's order: no padding in front, no slots) at n = 700 with 20 and 70 realisations -- one tile row
    under the band, trimmed and not: the objective against the oracle as test_taper_objective_vs_oracle holds it (1e-8), the
    gradient against tests/grad_taper_reference.py as test_value_and_gradient_vs_reference holds it (value 1e-9, each
    gradient 1e-7 of its largest entry)."""
    import cocons_amd as ca
    import grad_taper_reference as GT
    from cocons_amd import workloads as wl
    from cocons_amd.host import theta_table
    from test_gpu_parity import _problem as parity_problem, _taper_pattern
    n = 700
    locs, X, th, rng = parity_problem(n, seed=700 + n + r)
    th["mean"] = np.array([0.3, -0.2, 0.1])
    z = rng.standard_normal((n, r))
    ref_taper = _taper_pattern(locs, 0.25)
    pp = wl.par_pos_full()
    pp["mean"] = [True] * 3
    tv = np.r_[th["mean"], wl.theta_vector_from_lists(th, wl.par_pos_full())]
    tl = ca.getModelLists(tv, pp, "diff")
    assert all(np.allclose(tl[k], th[k], rtol=0, atol=1e-15) for k in th)
    lam = (0.1, 0.2, 0.3)
    fit = ca.CoconsTaperFit(locs, X, z, SL, *ref_taper)
    try:
        assert _layout(fit, 0) == [0, 0, 0, 1, trim]
        got = ca.GetNeg2loglikelihoodTaper(tv, pp, ref_taper, locs, X, SL, z, n, lam, fit=fit)
        gotp = ca.GetNeg2loglikelihoodTaperProfile(tv, pp, ref_taper, locs, X, SL, z, n, lam, fit=fit)
        v0 = fit.neg2loglik_core(tl)
        v, parts, gt, gq, gm = fit.neg2loglik_grad_core(tl)
        again = fit.neg2loglik_grad_core(tl)
        v1 = fit.neg2loglik_core(tl)
    finally:
        fit.close()
    want = oracle.GetNeg2loglikelihoodTaper(tv, pp, ref_taper, locs, X, SL, z, n, lam)
    wantp = oracle.GetNeg2loglikelihoodTaperProfile(tv, pp, ref_taper, locs, X, SL, z, n, lam)
    print("taper r=%d objective %.2e profile %.2e" % (r, abs(got - want) / abs(want), abs(gotp - wantp) / abs(wantp)))
    assert abs(got - want) <= 1e-8 * abs(want)
    assert abs(gotp - wantp) <= 1e-8 * abs(wantp)
    assert _same_bits(v1, v0)
    assert again[0] == v and all(np.array_equal(a, b) for a, b in zip(again[1:], (parts, gt, gq, gm)))
    assert abs(v - v0[0]) <= 1e-12 * abs(v0[0])
    assert np.max(np.abs(parts - v0[1])) <= 1e-12 * np.max(np.abs(v0[1]))
    f, rparts, rl, rq, rm = GT.neg2loglik_taper_grad(theta_table(tl), tl["mean"], locs, X, z, SL, ref_taper)
    print("taper r=%d gradient call: value %.2e" % (r, abs(v - f) / abs(f)))
    assert abs(v - f) <= 1e-9 * abs(f)
    for label, g, w in (("grad_theta", gt, rl + rq), ("grad_quad", gq, rq), ("grad_mean", gm, rm)):
        e = float(np.max(np.abs(g - w)) / np.max(np.abs(w)))
        print("taper r=%d %s %.2e of its largest entry" % (r, label, e))
        assert e <= 1e-7, (label, e)
