"""cocons_cv_taper_folds on the GPU -- cross-validation by folds of the tapered model S = T o C(theta) from one selected
inverse and one more band factorisation -- against the numpy statement of tests/cv_reference.py on the dense S of
tests/grad_taper_reference.py, built exactly as tests/test_gpu_cv_taper.py builds it.  The reference is brute force (one
Cholesky of the complement per fold).  Bound: 1e-8 in gap_e = max |resid - resid_ref| / sd_ref and gap_v = max |var - var_ref|
/ var_ref; on these inputs cv_kroute and cv_brute agree to 1.9e-12 / 1.5e-13 (cond S <= 2.4e3), so the bound leaves four
orders for the device.

Position modulo 64 (DESIGN.md 4n says a solved row depends on it): the folds are NOT placed so that a row's position in its
64-row strip is a function of the fold alone -- a packed tile puts a small fold behind whatever folds came before it.  That
it does not matter is shown here instead: test_bits permutes the labels (every fold moves to another tile and offset), merges
two folds (the folds behind them move up) and chunks the call, and asks for identical bits."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
import grad_taper_reference as GT  # noqa: E402
import taper_envelope_cases as TE  # noqa: E402
from test_gpu_grad_taper import _delta, _fit_memory, _setup, _taper_fit  # noqa: E402
from test_gpu_parity import _taper_pattern  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 1e-8


# --------------------------------------------------------------------------- problems, references (computed once, read-only)
@functools.lru_cache(maxsize=None)
def _problem(n, r):
    locs, X, th, z, _ = _setup(n, r)
    ref_taper = _taper_pattern(locs, _delta(n))
    for a in (locs, X, z):
        a.setflags(write=False)
    return locs, X, th, z, ref_taper


def _dense(th, locs, X, z, ref_taper, limits):
    from cocons_amd.host import theta_table
    S, _ = GT.taper_matrix(theta_table(th), locs, X, limits, ref_taper)
    S = np.tril(S) + np.tril(S, -1).T                   # (the library reads the lower triangle)
    return S, z - (X @ th["mean"])[:, None]


@functools.lru_cache(maxsize=None)
def _matrix(n, r):
    from cocons_amd import workloads as wl
    locs, X, th, z, ref_taper = _problem(n, r)
    out = _dense(th, locs, X, z, ref_taper, wl.SMOOTH_LIMITS)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _layouts(n, r):
    return CV.layouts(_problem(n, r)[0])


@functools.lru_cache(maxsize=None)
def _brute(n, r, layout):
    S, R = _matrix(n, r)
    return CV.cv_brute(S, R, _layouts(n, r)[layout])


def _check(tag, got, ref):
    ge, gv = CV.gaps(got[0], got[1], ref[0], ref[1])
    print("%s: gap_e %.3e gap_v %.3e (var %.3g .. %.3g)" % (tag, ge, gv, ref[1].min(), ref[1].max()))
    assert ge <= BOUND and gv <= BOUND, (tag, ge, gv)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _raw(fit_or_handle, L, th, lab, nfold, max_rows=0, n=None, r=1):
    """the C entry itself: (status, resid, var, stats5), the outputs filled with -7 beforehand"""
    from cocons_amd.host import _ip, _p, theta_table
    h = getattr(fit_or_handle, "_h", fit_or_handle)
    n = n if n is not None else fit_or_handle.n
    r = getattr(fit_or_handle, "r", r)
    resid, var = np.full((n, max(r, 1)), -7.0, order="F"), np.full(n, -7.0)
    stats = (ctypes.c_longlong * 5)(*([-7] * 5))
    lp = None if lab is None else _ip(np.ascontiguousarray(np.asarray(lab), dtype=np.int32))
    rc = L.cocons_cv_taper_folds(h, _p(theta_table(th)), _p(np.ascontiguousarray(th["mean"])), nfold, lp, max_rows,
                                 _p(resid), _p(var), stats)
    return rc, resid, var, list(stats)


# --------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("n,r", [(150, 1), (700, 2)])
def test_layouts_vs_brute_force(n, r):
    """two tiles and several: singleton labels, 10 random folds, 16 spatial blocks, 2 folds"""
    locs, X, th, z, ref_taper = _problem(n, r)
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        for name, lab in _layouts(n, r).items():
            got = fit.cv_core(th, lab)
            assert got[0].shape == (n, r) and got[1].shape == (n,)
            st = fit.last_cv_stats
            sizes = np.bincount(lab)
            sizes = sizes[sizes > 0]
            assert st[:3] == [int((sizes == 1).sum()), int(((sizes > 1) & (sizes <= 128)).sum()), int((sizes > 128).sum())], st
            assert (st[3] > 0) == bool((sizes > 1).any()) and st[4] > 0
            _check("n=%d r=%d %s" % (n, r, name), got, _brute(n, r, name))
    finally:
        fit.close()


MIXED = (1, 2, 16, 17, 127, 128, 129, 280)


def _mixed_labels(n, seed=5):
    assert sum(MIXED) == n
    return np.repeat(np.arange(len(MIXED)), MIXED)[np.random.default_rng(seed).permutation(n)]


def test_every_size_class_in_one_call():
    """n = 700, r = 3: folds of 1, 2, 16, 17, 127, 128, 129 and 280 -- the closed form, the four LDS classes at both of
    their edges, a large fold of two tiles with one row in the second, one of three tiles"""
    n, r = 700, 3
    locs, X, th, z, ref_taper = _problem(n, r)
    lab = _mixed_labels(n)
    S, R = _matrix(n, r)
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        got = fit.cv_core(th, lab)
        assert fit.last_cv_stats[:3] == [1, 5, 2]
    finally:
        fit.close()
    _check("mixed sizes", got, CV.cv_brute(S, R, lab))


def test_packed_band_buffer_and_several_gram_groups():
    """n = 1500: the packed band buffer, nt = 12 tile columns, so two Gram groups at depth 8; 10 random folds (150 each: two
    tiles) and 2 folds of 750"""
    n, r = 1500, 1
    locs, X, th, z, ref_taper = _problem(n, r)
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        assert fit.krige_taper_info()["nt"] == 12
        for name in ("random10", "two"):
            got = fit.cv_core(th, _layouts(n, r)[name])
            _check("n=1500 %s" % name, got, _brute(n, r, name))
    finally:
        fit.close()


@functools.lru_cache(maxsize=None)
def _wide_dense(base):
    """(S, R) of a case wider than eight tile rows: the lines of _dense, 9 s and more at these sizes, so computed once for
    this file and tests/test_gpu_taper_envelopes.py"""
    from test_gpu_taper_envelopes import _ref_matrix
    return _ref_matrix(base)


@functools.lru_cache(maxsize=None)
def _wide_brute(base, layout):
    """cv_brute on the layout `layout` of _wide_layouts (or on the 10 random folds of test_irregular_envelopes)"""
    p = TE.problem(base)
    lab = np.random.default_rng(17).permutation(p.n) % 10 if layout == "irregular" else _wide_layouts(base)[layout]
    return CV.cv_brute(*_wide_dense(base), lab)


@functools.lru_cache(maxsize=None)
def _wide_layouts(base):
    """CV.layouts without leave-one-out: 10 random folds, the spatial blocks, 2 folds -- 28 folds at most, each one Cholesky
    of order n - |fold| for brute force (leave-one-out, n folds, is tests/test_gpu_taper_envelopes.py's, with a stride)"""
    out = CV.layouts(TE.problem(base).locs)
    del out["loo"]
    assert sum(np.unique(lab).size for lab in out.values()) <= 64
    return out


@pytest.mark.parametrize("name,depth", [("clusters", None), ("chain", None), ("chain", "1"), ("hub_caller", None),
                                        ("islands", None), ("flat9", None), ("flat9", "1"), ("flat9", "3"), ("tall", None),
                                        ("tall", "3"), ("tall_rcm", "1"), ("flat10_long", None), ("flat10_long", "3")])
def test_irregular_envelopes(monkeypatch, name, depth):
    """10 random folds on the envelopes of tests/taper_envelope_cases.py: clusters (n = 1281, a ragged envelope), chain (W = 4 of
    10; at Gram depth 1 the ring has W slots and wraps), hub_caller (W = nt, unpacked), islands (S diagonal: resid = R and
    var = diag S); and on the bands wider than eight tile rows, flat9, tall and tall_rcm (W = 10, 12, 11 of nt = 14, 15, 15)
    and flat10_long (W = 10 of 20): at the default depth of 8 only flat10_long's ring of W + 7 slots is shorter than nt; at
    depth 3 every one wraps at W + 2, a modulus that is not W, and at depth 1 at W itself"""
    from test_gpu_taper_envelopes import _assert_shape, _fit
    p = TE.problem(name)
    if name in TE.WIDE:
        S, R = _wide_dense(p.base)
    else:
        S, R = _dense(p.theta, p.locs, p.X, p.z, p.ref_taper, TE.SMOOTH_LIMITS)
    lab = np.random.default_rng(17).permutation(p.n) % 10
    fit = _fit(monkeypatch, p)
    try:
        _, nt, _, W = _assert_shape(fit, p)
        if name == "chain":
            assert (W, nt) == (4, 10)
        if depth:
            monkeypatch.setenv("COCONS_CV_GRAM_DEPTH", depth)
        if name in TE.WIDE:
            assert W > 8
            if depth or name == "flat10_long":
                assert W + int(depth or 8) - 1 < nt, (W, nt, depth)          # a ring shorter than the matrix: it wraps
        got = fit.cv_core(p.theta, lab)
    finally:
        fit.close()
    ref = _wide_brute(p.base, "irregular") if name in TE.WIDE else CV.cv_brute(S, R, lab)
    _check("%s depth %s" % (name, depth or "default"), got, ref)
    if name == "islands":
        _check("islands: resid = R, var = diag S", got, (R, np.diag(S).copy()))


@pytest.mark.parametrize("name", ["flat9", "tall"])
def test_layouts_on_wide_bands(monkeypatch, name):
    """the layouts of CV.layouts but leave-one-out (_wide_layouts) on flat9 and tall against brute force, at BOUND; the spatial
    blocks put whole tile columns of the caller's order into one fold (flat9: sorted by x; tall: the clique is one block or
    two), so large folds span the wide part of the band"""
    from test_gpu_taper_envelopes import _assert_shape, _fit
    p = TE.problem(name)
    fit = _fit(monkeypatch, p)
    try:
        _, nt, _, W = _assert_shape(fit, p)
        for layout, lab in _wide_layouts(p.base).items():
            got = fit.cv_core(p.theta, lab)
            sizes = np.bincount(lab)
            _check("%s (nt %d, W %d) %s, %d folds of %d .. %d" % (name, nt, W, layout, (sizes > 0).sum(), sizes[sizes > 0].min(),
                                                                sizes.max()), got, _wide_brute(p.base, layout))
    finally:
        fit.close()


@pytest.mark.parametrize("together", [True, False])
def test_duplicated_location(monkeypatch, together):
    """the duplicated-location case of test_gpu_cv_taper.py with the pair in one fold and in two"""
    from cocons_amd import workloads as wl
    monkeypatch.setenv("COCONS_TAPER_RCM", "0")
    n, r = 700, 1
    locs, X, th, z, _ = _setup(n, r, seed=31)
    locs[400] = locs[5]
    X[400] = X[5]
    X[5] = X[5] + [0.0, 0.5, 0.0]
    ref_taper = _taper_pattern(locs, 0.25)
    lab = np.random.default_rng(3).permutation(n) % 10
    if together:
        lab[400] = lab[5]
    else:
        lab = CV._apart(lab, 5, 400)
    assert (lab[400] == lab[5]) == together
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        got = fit.cv_core(th, lab)
    finally:
        fit.close()
    S, R = _dense(th, locs, X, z, ref_taper, wl.SMOOTH_LIMITS)
    ref = CV.cv_brute(S, R, lab)
    _check("duplicate, %s" % ("one fold" if together else "two folds"), got, ref)
    if not together:
        assert ref[1][[5, 400]].max() < np.median(ref[1])      # (each of the two is predicted from the other)


# --------------------------------------------------------------------------- bits
def test_bits(monkeypatch):
    n, r = 700, 2
    locs, X, th, z, ref_taper = _problem(n, r)
    rng = np.random.default_rng(23)
    order = rng.permutation(n)
    # folds of 16, 129, 70 and 74, the rest in folds of 40 or so and a few singletons
    lab = np.empty(n, dtype=int)
    cuts = np.cumsum([0, 16, 129, 70, 74])
    for k in range(4):
        lab[order[cuts[k]:cuts[k + 1]]] = k
    rest = order[cuts[-1]:]
    lab[rest[:5]] = 4 + np.arange(5)
    lab[rest[5:]] = 9 + np.arange(rest.size - 5) % 10
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        L = fit._L
        base = fit.cv_core(th, lab)
        stats0 = fit.last_cv_stats
        assert _same(base, fit.cv_core(th, lab)), "a repeated call"
        # fold = NULL and all-singleton labels are cocons_cv_taper
        loo = fit.cv_core(th)
        rc, e, v, st = _raw(fit, L, th, None, 0)
        assert rc == 0 and _same((e, v), loo) and st[:4] == [n, 0, 0, 0]
        rc, e, v, st = _raw(fit, L, th, rng.permutation(n), n)
        assert rc == 0 and _same((e, v), loo) and st[:4] == [n, 0, 0, 0]
        # other names for the same folds: every fold moves to another tile and another offset in it
        relabel = rng.permutation(int(lab.max()) + 1)
        assert _same(base, fit.cv_core(th, relabel[lab])), "permuted labels"
        # the folds of 70 and 74 merged into one of 144: the folds of 16 and 129 keep their bits
        merged = np.where(lab == 3, 2, lab)
        got = fit.cv_core(th, merged)
        assert fit.last_cv_stats[2] == stats0[2] + 1
        keep = (lab == 0) | (lab == 1)
        assert np.array_equal(got[0][keep], base[0][keep]) and np.array_equal(got[1][keep], base[1][keep]), "merged folds"
        assert not np.array_equal(got[1][lab == 2], base[1][lab == 2])
        # chunks of one tile
        assert stats0[3] == 1
        assert _same(base, fit.cv_core(th, lab, max_rows=128)), "max_rows = 128"
        assert fit.last_cv_stats[3] > 1 and fit.last_cv_stats[:3] == stats0[:3]
        # one tile column per Gram launch
        monkeypatch.setenv("COCONS_CV_GRAM_DEPTH", "1")
        assert _same(base, fit.cv_core(th, lab)), "Gram depth 1"
        monkeypatch.setenv("COCONS_CV_GRAM_DEPTH", "17")
        rc, e, v, st = _raw(fit, L, th, lab, int(lab.max()) + 1)
        assert rc == -1 and np.all(e == -7.0) and np.all(v == -7.0)
    finally:
        fit.close()


# --------------------------------------------------------------------------- the handle's state
def test_state_of_the_handle_is_left_alone():
    from test_gpu_krige_taper import _pred_taper
    n, r, m = 700, 2, 150
    locs, X, th, z, ref_taper = _problem(n, r)
    rng = np.random.default_rng(41)
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = np.column_stack([np.ones(m), rng.standard_normal(m), rng.standard_normal(m)])
    pt = _pred_taper(lp, locs, _delta(n))
    lab = _mixed_labels(n, seed=6)
    th2 = {k: np.array(v, dtype=float) for k, v in th.items()}
    th2["scale"] = th2["scale"] + np.array([0.15, 0.0, 0.0])
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        fit.krige_taper_prepare(th2, z_col=1)
        before = (fit.neg2loglik_core(th), fit.neg2loglik_grad_core(th), fit.cv_core(th), fit.krige_taper_core(lp, Xp, pt))
        info0 = fit.krige_taper_info()
        fit.cv_core(th, lab)
        mem1 = _fit_memory(fit)
        fit.cv_core(th, lab, max_rows=128)
        assert _fit_memory(fit) == mem1
        after = (fit.neg2loglik_core(th), fit.neg2loglik_grad_core(th), fit.cv_core(th), fit.krige_taper_core(lp, Xp, pt))
        assert fit.krige_taper_info() == info0
        assert fit.engine_state()["retries"] == 0
    finally:
        fit.close()
    assert before[0][0] == after[0][0] and np.array_equal(before[0][1], after[0][1])
    assert before[1][0] == after[1][0] and all(np.array_equal(a, b) for a, b in zip(before[1][1:], after[1][1:]))
    assert _same(before[2], after[2]) and _same(before[3], after[3])


# --------------------------------------------------------------------------- failures and refusals
def test_failures_and_refusals_on_the_device():
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    from cocons_amd.host import _f, _p, theta_table
    n, r = 150, 1
    locs, X, th, z, ref_taper = _problem(n, r)
    lab = np.arange(n) % 10
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        L = fit._L
        th_bad = {k: np.array(v, dtype=float).copy() for k, v in th.items()}
        th_bad["std.dev"][0] = -np.inf
        th_bad["nugget"][0] = -np.inf
        e1, v1 = np.full((n, r), -7.0, order="F"), np.full(n, -7.0)
        want = L.cocons_cv_taper(fit._h, _p(theta_table(th_bad)), _p(np.ascontiguousarray(th_bad["mean"])), _p(e1), _p(v1))
        rc, e, v, st = _raw(fit, L, th_bad, lab, 10)
        assert want > 0 and rc == want, (rc, want)
        assert np.all(e == -7.0) and np.all(v == -7.0) and st == [-7] * 5 and np.all(e1 == -7.0)
        good = fit.cv_core(th, lab)                      # the handle recovers
        for bad, nfold, what in ((np.where(np.arange(n) == 7, 10, lab), 10, "label 10 of observation 7"),
                                 (np.where(np.arange(n) == 7, -1, lab), 10, "label -1 of observation 7"),
                                 (np.zeros(n, dtype=int), 3, "fold 0 holds all")):
            rc, e, v, st = _raw(fit, L, th, bad, nfold)
            assert rc == -1 and _lib.last_error().startswith("cocons_cv_taper_folds:") and what in _lib.last_error()
            assert np.all(e == -7.0) and np.all(v == -7.0) and st == [-7] * 5
        assert _same(good, fit.cv_core(th, lab))
    finally:
        fit.close()
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        rc, e, v, _ = _raw(dense, dense._L, th, lab, 10)
        assert rc == -1 and "not a taper fit" in _lib.last_error() and np.all(e == -7.0) and np.all(v == -7.0)
    finally:
        dense.close()
    # a handle without z (a taper handle always has one: cocons_fit_create_taper asks for r >= 1)
    L = _lib.load()
    lf, Xf, sl = _f(locs), _f(X), np.array(wl.SMOOTH_LIMITS, float)
    h = L.cocons_fit_create(n, 3, 0, 0, _p(lf), _p(Xf), None, None, _p(sl), -1)
    assert h
    try:
        rc, e, v, _ = _raw(h, L, th, lab, 10, n=n)
        assert rc == -1 and _lib.last_error().startswith("cocons_cv_taper_folds:") and np.all(e == -7.0) and np.all(v == -7.0)
    finally:
        L.cocons_fit_destroy(h)


# --------------------------------------------------------------------------- layouts of the factorisation buffer
@pytest.mark.parametrize("switch", ["COCONS_TAPER_PACKED", "COCONS_TAPER_BAND"])
def test_buffer_layouts_meet_the_bound(monkeypatch, switch):
    n, r = 700, 2
    locs, X, th, z, ref_taper = _problem(n, r)
    monkeypatch.setenv(switch, "0")
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        for name in ("random10", "two"):
            _check("%s=0 %s" % (switch, name), fit.cv_core(th, _layouts(n, r)[name]), _brute(n, r, name))
    finally:
        fit.close()


# --------------------------------------------------------------------------- host and glue
def test_host_and_glue():
    """host.cocoCV_sparse(fold=...) with string labels, with and without a handle, equals cv_core; the glue's
    _cocons_hip_cv_taper_folds through the R stub equals the Python call bit for bit"""
    from cocons_amd import host, workloads as wl
    from test_glue_exec import RStub
    n, r = 150, 2
    locs, X, th, z, ref_taper = _problem(n, r)
    lab = np.random.default_rng(2).permutation(n) % 7
    names = np.array(["f%d" % k for k in lab])
    fit = _taper_fit(locs, X, z, ref_taper)
    try:
        norm = np.unique(names, return_inverse=True)[1]
        want = fit.cv_core(th, norm)
        out = host.cocoCV_sparse(th, locs, X, wl.SMOOTH_LIMITS, z, ref_taper, fit=fit, fold=names)
        chunked = fit.cv_core(th, norm, max_rows=128)
    finally:
        fit.close()
    own = host.cocoCV_sparse(th, locs, X, wl.SMOOTH_LIMITS, z, ref_taper, fold=names)
    for o in (out, own):
        assert np.array_equal(o["resid"], want[0]) and np.array_equal(o["sd.pred"], np.sqrt(want[1]))
        assert np.array_equal(o["mean.pred"], z - want[0])
    assert _same(want, chunked)
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_cv_taper_folds") == 5
    ci, rp, ent = ref_taper
    h = R.call("_cocons_hip_fit_create_taper", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer(ci), R.integer(rp), R.real(ent))
    for mr in (0, 128):
        st, got = R.value(R.call("_cocons_hip_cv_taper_folds", h, R.theta(th), R.real(th["mean"]), R.integer(norm), R.integer([mr])))
        assert int(st[0]) == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    st, got = R.value(R.call("_cocons_hip_cv_taper_folds", h, R.theta(th), R.real(th["mean"]), R.nil, R.integer([0])))
    st2, loo = R.value(R.call("_cocons_hip_cv_taper", h, R.theta(th), R.real(th["mean"])))
    assert int(st[0]) == 0 and int(st2[0]) == 0 and np.array_equal(got[0], loo[0]) and np.array_equal(got[1], loo[1])
    R.call("_cocons_hip_fit_close", h)
    R.L.stub_gc(0, None)
