"""U^-T on a Vecchia fit on the GPU (cocons_vecchia_unwhiten_t, cocons_vecchia_cov_mult, cocons_vecchia_cov_cols,
cocons_vecchia_schedule_t, cocoPredict_vecchia_joint) against tests/vecchia_cov_reference.py in long double on the oracle's
matrices: the problem of test_gpu_dense_sizes.problem, the tables of test_gpu_vecchia.table, and star and chain tables that put
a transposed list on every side of the tiers' boundaries (the threshold read through cocons_debug_vecchia_solve_t_tiers).

Bound of every comparison with a reference: the project's parity bound, PARITY = 1e-8 of test_gpu_dense_sizes, relative to the
largest magnitude of the compared array.  (The restatement in double differs from long double by at most 4.7e-16 at n = 40,
tests/test_vecchia_cov_reference.py: the bound leaves seven orders for the device's own rounding and hides nothing.)  Schedules
are compared as integers, bits with np.array_equal.  Every test prints its worst error on one line that starts with
`vecchia-cov-report`; the measured figures stand in tests/golden/VECCHIA_COV_REPORT.md."""
import contextlib
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_cov_reference as VC  # noqa: E402
import vecchia_reference as VR  # noqa: E402
import vecchia_sim_reference as VS  # noqa: E402
from test_gpu_dense_sizes import PARITY, problem  # noqa: E402
from test_gpu_vecchia import MS, SIZES, _duplicate_site, _fit, _theta, table  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCH = "COCONS_VECCHIA_SOLVE_T_FUSE"
C = 17                                          # columns of the value tests: two full column groups and one of a single column


def _report(what, case, err):
    print("vecchia-cov-report gpu | %s | %s | %.2e" % (what, case, err))


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


@contextlib.contextmanager
def _switch(value):
    """the library reads the switch at every call"""
    old = os.environ.get(SWITCH)
    try:
        if value is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = value
        yield
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


@functools.lru_cache(maxsize=None)
def tiers():
    """{"wide": a list of MORE than this many rows goes to the workgroup tier, "threads", "cols", "fuse_items"} (host only)"""
    from cocons_amd import _lib
    out = (ctypes.c_int * 4)()
    assert _lib.load().cocons_debug_vecchia_solve_t_tiers(out) == 0
    return dict(zip(("wide", "threads", "cols", "fuse_items"), (int(v) for v in out)))


@functools.lru_cache(maxsize=None)
def columns(n, c=C):
    W = np.asfortranarray(np.random.default_rng(2000 + n).standard_normal((n, c)))
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def special(kind, n):
    """star: every later row names row 1 only (list(0) has n - 1 entries, depth 2).  chain: row i names i - 1 (depth n, fused
    runs).  lone: nobody names anybody."""
    nn = np.zeros((n, 1), dtype=np.int32, order="F")
    if kind == "star":
        nn[1:, 0] = 1
    elif kind == "chain":
        nn[1:, 0] = np.arange(1, n)
    nn.setflags(write=False)
    return nn


def _table_of(spec):
    return special(*spec) if isinstance(spec[0], str) else table(*spec)


def _mid(n):
    return n // 2


@functools.lru_cache(maxsize=None)
def reference(spec):
    """long double, computed once per table: (U^-T W for the C columns, cov_mult of the first 3 columns for n_fixed = 0, the
    same for n_fixed = n // 2 on the rows behind it), as doubles"""
    nn = _table_of(spec)
    n = nn.shape[0]
    coef = VS.coefficients(problem(n)[6], nn, np.longdouble)
    W = columns(n)
    nf = _mid(n)
    out = tuple(np.asarray(a, dtype=float) for a in (VC.solve_t(coef, nn, W), VC.cov_mult(None, nn, W[:, :3], coef=coef),
                                                     VC.cov_mult(None, nn, W[nf:, :3], nf, coef=coef)))
    for a in out:
        a.setflags(write=False)
    return out


def _spec_fit(spec):
    nn = _table_of(spec)
    return _fit(nn.shape[0], nn.shape[1], nn=nn)


def _check_values(spec, case):
    n = _table_of(spec).shape[0]
    th, W = problem(n)[2], columns(n)
    nf = _mid(n)
    ref_t, ref_c, ref_f = reference(spec)
    f = _spec_fit(spec)
    try:
        v = f.unwhiten_t_core(th, W)
        back = f.whiten_t_core(th, v)[0]
        forth = f.unwhiten_t_core(th, f.whiten_t_core(th, W)[0])
        cm = f.cov_mult_core(th, W[:, :3])
        cf = f.cov_mult_core(th, W[nf:, :3], n_fixed=nf)
        idx = np.unique(np.array([nf + 1, n, (nf + n + 1) // 2, n]))
        cols = f.cov_cols_core(th, idx, n_fixed=nf)
        units = np.zeros((n - nf, idx.size), order="F")
        units[idx - nf - 1, np.arange(idx.size)] = 1.0
        by_mult = f.cov_mult_core(th, units, n_fixed=nf)
    finally:
        f.close()
    errs = dict(unwhiten_t=_rel(v, ref_t), whiten_t_of=_rel(back, W), of_whiten_t=_rel(forth, W), cov_mult=_rel(cm, ref_c),
                       cov_mult_fixed=_rel(cf, ref_f))
    for k, e in errs.items():
        _report(k, case, e)
    assert max(errs.values()) < PARITY, errs
    assert np.array_equal(cols, by_mult)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_values_on_the_tables_of_the_likelihood_tests(n, m):
    """n = 1, n = 2, rows with fewer than m predecessors, the full 64-row block (n = 65, m = 63: row 1 is named by 63 rows or
    more), the 64 / 65 seam"""
    _check_values((n, m), "n%d m%d" % (n, m))


def test_values_n200_m63_and_holes():
    _check_values((200, 63), "n200 m63")
    _check_values((65, 10, True), "holes n65 m10")


def test_n2_without_a_neighbour():
    _check_values(("lone", 2), "lone n2")


@pytest.mark.parametrize("rows", (63, 64, 65, 128, 129))
def test_star_tables_around_the_wavefront(rows):
    """list(0) of 63, 64, 65, 128, 129 entries: a lane with nothing, every lane one entry, one lane with two, .. (one-wave tier)"""
    _check_values(("star", rows + 1), "star list %d" % rows)


@pytest.mark.parametrize("off", (-1, 0, 1))
def test_star_tables_around_the_wide_tier(off):
    """list(0) of threshold - 1 and threshold entries (one wavefront) and threshold + 1 (the workgroup)"""
    rows = tiers()["wide"] + off
    spec = ("star", rows + 1)
    _check_values(spec, "star list %d (threshold %+d)" % (rows, off))
    f = _spec_fit(spec)
    try:
        with _switch("0"):
            s = f.schedule_t()
    finally:
        f.close()
    # without fusing: level 1 (the leaves) is one launch, level 2 (row 1) one launch of whichever tier it is in
    assert (s["depth"], s["widest"], s["launches"]) == (2, rows, 2)


def test_star_n5000_and_chain_n300():
    """a list of 4999 entries (five entries a thread of the workgroup, the last ones fewer) and a depth of 300 (fused runs)"""
    _check_values(("star", 5000), "star n5000")
    _check_values(("chain", 300), "chain n300")
    f = _spec_fit(("chain", 300))
    try:
        s = f.schedule_t()
        with _switch("0"):
            s0 = f.schedule_t()
    finally:
        f.close()
    assert (s["depth"], s["widest"], s["launches"], s0["launches"]) == (300, 1, 1, 300)


SCHEDULES = [(n, m) for n in SIZES for m in MS] + [(200, 63), (65, 10, True), ("star", 65), ("star", 130), ("chain", 300), ("lone", 2)]


@pytest.mark.parametrize("spec", SCHEDULES, ids=str)
def test_schedules_equal_the_reference_exactly(spec):
    nn = _table_of(spec)
    n = nn.shape[0]
    f = _spec_fit(spec)
    try:
        for n_fixed in sorted({0, 1, n // 2, n - 1}):
            if not 0 <= n_fixed < n:
                continue
            want = VC.tlevels(nn, n_fixed)
            got = f.schedule_t(n_fixed)
            assert got["levels"].dtype == np.int32 and np.array_equal(got["levels"], want), (spec, n_fixed)
            assert got["depth"] == int(want.max()) == f.schedule(n_fixed)["depth"]
            assert got["widest"] == int(np.bincount(want[n_fixed:]).max())
            assert 1 <= got["launches"] <= got["depth"]
            with _switch("0"):
                # one launch per level and tier; no list here is beyond the threshold
                assert f.schedule_t(n_fixed)["launches"] == got["depth"]
    finally:
        f.close()
    _report("schedule_t: levels, depth, widest", str(spec), 0.0)


BITS = [(641, 30), (65, 63), (300, 10), ("star", 130), ("chain", 300)]


@pytest.mark.parametrize("spec", BITS, ids=str)
def test_bits_repeat_columns_and_the_fuse_switch(spec):
    n = _table_of(spec).shape[0]
    th, W = problem(n)[2], columns(n)
    f = _spec_fit(spec)
    try:
        a, b = f.unwhiten_t_core(th, W), f.unwhiten_t_core(th, W)
        ca, cb = f.cov_mult_core(th, W), f.cov_mult_core(th, W)
        singles = {k: (f.unwhiten_t_core(th, W[:, k]), f.cov_mult_core(th, W[:, k])) for k in (0, 7, 8, 16)}
        narrower = {c: (f.unwhiten_t_core(th, W[:, :c]), f.cov_mult_core(th, W[:, :c])) for c in (8, 9)}
        with _switch("0"):
            c, cc = f.unwhiten_t_core(th, W), f.cov_mult_core(th, W)
        g = _spec_fit(spec)
        try:
            with _switch("0"):
                d = g.unwhiten_t_core(th, W)                # a handle that never saw the default
        finally:
            g.close()
    finally:
        f.close()
    _report("bits: repeat, columns 1 / 8 / 9 / 17, fuse off", str(spec), float(np.max(np.abs(a - c))))
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    assert np.array_equal(ca, cb) and np.array_equal(ca, cc)
    for k, (u, v) in singles.items():
        assert np.array_equal(u[:, 0], a[:, k]) and np.array_equal(v[:, 0], ca[:, k]), k
    for c_, (u, v) in narrower.items():
        assert np.array_equal(u, a[:, :c_]) and np.array_equal(v, ca[:, :c_]), c_


@pytest.mark.parametrize("kind", ("table", "wide star", "chain"))
def test_rows_behind_n_fixed_do_not_see_n_fixed(kind):
    """The transposed part of cocons_vecchia_cov_mult is not exposed, so the property is checked through the entries that are:
    on a handle with z = 0 and a zero mean, cocons_sim_vecchia with n_fixed runs the forward solve of cov_mult with the fixed
    rows at zero on whatever columns it is given.  Given rows >= n_fixed of cocons_vecchia_unwhiten_t (solved with n_fixed = 0,
    on columns that agree behind n_fixed and are arbitrary in front), it must return cov_mult(n_fixed)'s bits."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    spec = {"table": (300, 30), "wide star": ("star", tiers()["wide"] + 300), "chain": ("chain", 300)}[kind]
    nn = _table_of(spec)
    n = nn.shape[0]
    locs, X, th0 = problem(n)[:3]
    th = _theta(th0)
    th["mean"] = np.zeros_like(th0["mean"])
    W = columns(n)[:, :3]
    f = ca.CoconsVecchiaFit(locs, X, np.zeros(n), wl.SMOOTH_LIMITS, nn)
    try:
        full = f.unwhiten_t_core(th, W)
        for nf in sorted({1, n // 2, n - 1}):
            want = f.cov_mult_core(th, W[nf:], n_fixed=nf)
            got = f.sim_core(th, full[nf:], n_fixed=nf)
            assert np.array_equal(got, want), (spec, nf)
    finally:
        f.close()
    _report("bits: rows behind n_fixed", str(spec), 0.0)


def test_exact_with_all_predecessors_against_the_dense_model():
    """n = 64, m = 63, every predecessor: the model's covariance is Sigma itself -- cocons_cov_rows of a dense handle -- and with
    24 rows fixed the conditional covariance of the other 40"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, nf = 64, 24
    locs, X, th, z = (np.array(a[:n]) if isinstance(a, np.ndarray) else a for a in problem(65)[:4])
    X, z = np.asfortranarray(X), np.asfortranarray(z)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    d = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        cols = f.cov_cols_core(th, np.arange(1, n + 1))
        S = d.cov_rows(th, np.arange(n))
        cond = f.cov_cols_core(th, np.arange(nf + 1, n + 1), n_fixed=nf)
    finally:
        f.close()
        d.close()
    want = S[nf:, nf:] - S[nf:, :nf] @ np.linalg.solve(S[:nf, :nf], S[:nf, nf:])
    errs = (_rel(cols, S.T), _rel(cond, want))
    _report("exact: cov_rows of a dense handle, numpy conditional covariance", "n64 m63 fixed 0 / 24", max(errs))
    assert max(errs) < PARITY, errs


def test_grouped_coefficients_give_the_same_bits():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n, m = 300, 10
    locs, X, th, z = problem(n)[:4]
    W = columns(n)[:, :3]
    f = ca.CoconsVecchiaFit.from_groups(locs, X, z, wl.SMOOTH_LIMITS, table(n, m))
    plain = _fit(n, m)
    try:
        idx = np.array([n, 151, 151])
        for nf in (0, 150):
            assert np.array_equal(f.cov_mult_core(th, W[nf:], n_fixed=nf, grouped=True), f.cov_mult_core(th, W[nf:], n_fixed=nf))
            assert np.array_equal(f.cov_cols_core(th, idx, n_fixed=nf, grouped=True), f.cov_cols_core(th, idx, n_fixed=nf))
        assert np.array_equal(f.unwhiten_t_core(th, W, grouped=True), f.unwhiten_t_core(th, W))
        # a handle without a plan
        out = np.full((n, 3), 7.0, order="F")
        T = host.theta_table(th)
        assert plain._L.cocons_vecchia_unwhiten_t(plain._h, host._p(T), 1, 3, host._p(np.asfortranarray(W)), host._p(out)) == -1
        assert _lib.last_error().startswith("cocons_vecchia_unwhiten_t:") and np.all(out == 7.0)
    finally:
        f.close()
        plain.close()
    _report("bits: grouped against ungrouped", "n%d m%d" % (n, m), 0.0)


def test_new_entries_between_the_others_keep_every_result_at_its_fresh_handle_bits():
    """value, whiten, unwhiten, whiten_t, cv and sim share V->aos, V->B, V->W and the coefficients with the new entries"""
    n, m = 300, 30
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    W = columns(n)[:, :3]

    def others(f):
        return [np.concatenate([[f.neg2loglik_core(th)[0]], f.neg2loglik_core(th)[1]]),
                np.concatenate([a.ravel() for a in f.whiten_core(th, Rz)]),
                f.unwhiten_core(th, W),
                np.concatenate([a.ravel() for a in f.whiten_t_core(th, W)]),
                np.concatenate([a.ravel() for a in f.cv_core(th)]),
                f.sim_core(th, W[64:, :1], n_fixed=64, z_col=1),
                f.schedule(64)["levels"]]

    def new(f):
        return [f.unwhiten_t_core(th, W), f.cov_mult_core(th, W), f.cov_mult_core(th, W[64:], n_fixed=64),
                f.cov_cols_core(th, [70, 300, 70], n_fixed=64), f.schedule_t(64)["levels"], f.schedule_t()["levels"]]

    a, b, c = _fit(n, m), _fit(n, m), _fit(n, m)
    try:
        fresh_others, fresh_new = others(a), new(b)
        mixed_new = new(c)
        mixed_others = others(c)
        again_new = new(c)
        interleaved = []
        for k in range(len(fresh_others)):
            interleaved.append(others(c)[k])
            c.cov_mult_core(th, W[100:, :1], n_fixed=100)
    finally:
        for f in (a, b, c):
            f.close()
    for got in (mixed_new, again_new):
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh_new))
    for got in (mixed_others, interleaved):
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh_others))
    _report("order of calls", "n%d m%d" % (n, m), 0.0)


def test_failing_block_returns_its_row_and_fixed_in_front_it_does_not_fail():
    """test_gpu_vecchia's failing block (row 58, a numerical refusal, not a device fault)"""
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    locs, X, th0, z, nn = _duplicate_site(False)
    n = 65
    nn[58:][nn[58:] == 58] = 0                     # nobody behind the duplicate names it: its own block is the only one that fails
    slope = np.array([0.0, 0.3, -0.2])
    up = float((X[57] - X[40]) @ slope) > 0
    good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
    W = np.asfortranarray(columns(n)[:, :3])
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    g = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        L, T = f._L, host.theta_table(bad)
        fresh = g.unwhiten_t_core(good, W)
        out = np.full((n, 3), 7.0, order="F")
        assert L.cocons_vecchia_unwhiten_t(f._h, host._p(T), 0, 3, host._p(W), host._p(out)) == 58
        assert L.cocons_vecchia_cov_mult(f._h, host._p(T), 0, 0, 3, host._p(W), host._p(out)) == 58
        idx = np.array([60, 65], dtype=np.int32)
        assert L.cocons_vecchia_cov_cols(f._h, host._p(T), 0, 57, 2, host._ip(idx), host._p(out)) == 58
        assert np.all(out == 7.0)
        with pytest.raises(_lib.CholeskyError) as e:
            f.cov_mult_core(bad, W)
        assert e.value.minor == 58
        # the duplicate among the fixed rows: its block is never factored
        ok = f.cov_mult_core(bad, W[58:], n_fixed=58)
        assert np.all(np.isfinite(ok))
        assert np.array_equal(f.cov_cols_core(bad, [60, 65], n_fixed=58), f.cov_mult_core(bad, np.eye(n - 58)[:, [1, 6]], n_fixed=58))
        assert np.array_equal(f.unwhiten_t_core(good, W), fresh)
    finally:
        f.close()
        g.close()
    _report("failing block", "n65 row 58", 0.0)


def test_refusals_that_need_a_handle_and_the_bytes_of_the_handle():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n = 65
    locs, X, th, z = problem(n)[:4]
    T = host.theta_table(th)
    W, out = np.asfortranarray(columns(n)[:, :3]), np.full((n, 3), 7.0, order="F")
    out4 = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    vec = _fit(n, 10)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        L = vec._L
        for n_fixed in (n, n + 5):
            assert L.cocons_vecchia_cov_mult(vec._h, host._p(T), 0, n_fixed, 3, host._p(W), host._p(out)) == -1
            assert _lib.last_error() == "cocons_vecchia_cov_mult: n_fixed = %d is outside 0 .. 64" % n_fixed
            idx = np.array([n_fixed + 1], dtype=np.int32)
            assert L.cocons_vecchia_cov_cols(vec._h, host._p(T), 0, n_fixed, 1, host._ip(idx), host._p(out)) == -1
            assert _lib.last_error() == "cocons_vecchia_cov_cols: n_fixed = %d is outside 0 .. 64" % n_fixed
            assert L.cocons_vecchia_schedule_t(vec._h, n_fixed, None, out4) == -1
            assert _lib.last_error() == "cocons_vecchia_schedule_t: n_fixed = %d is outside 0 .. 64" % n_fixed
        for bad in ([66], [5, 66], [0], [10]):                      # beyond n, and not behind n_fixed = 10
            idx = np.array(bad, dtype=np.int32)
            assert L.cocons_vecchia_cov_cols(vec._h, host._p(T), 0, 10, idx.size, host._ip(idx), host._p(out)) == -1
            assert _lib.last_error().startswith("cocons_vecchia_cov_cols: idx["), _lib.last_error()
        for name, call in (("cocons_vecchia_unwhiten_t", lambda h: L.cocons_vecchia_unwhiten_t(h, host._p(T), 0, 3, host._p(W), host._p(out))),
                           ("cocons_vecchia_cov_mult", lambda h: L.cocons_vecchia_cov_mult(h, host._p(T), 0, 0, 3, host._p(W), host._p(out))),
                           ("cocons_vecchia_cov_cols", lambda h: L.cocons_vecchia_cov_cols(h, host._p(T), 0, 0, 1,
                                                                                         host._ip(np.array([3], dtype=np.int32)), host._p(out))),
                           ("cocons_vecchia_schedule_t", lambda h: L.cocons_vecchia_schedule_t(h, 0, None, out4))):
            assert call(dense._h) == -1
            assert _lib.last_error().startswith(name + ": not a Vecchia fit"), _lib.last_error()
        assert np.all(out == 7.0) and list(out4) == [-7] * 4
        # the transposed schedule is the handle's and is counted
        before = vec.info()["bytes"]
        vec.cov_cols_core(th, [1, 65])
        s = vec.schedule_t()
        assert s["bytes"] >= 5 * n * 4 and vec.info()["bytes"] - before >= s["bytes"]
    finally:
        vec.close()
        dense.close()


def test_joint_prediction_function():
    """60 observations and 12 new sites: m = 71 is refused, m = 63 accepted; the mean is cocoSim_cond_vecchia's with zero
    errors; the covariance is symmetric; with every predecessor named (40 observations, m = 51) it is the dense model's"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    n, mp = 60, 12
    locs, X, th, z, lp, Xp = (np.array(a) if isinstance(a, np.ndarray) else a for a in problem(65)[:6])
    locs, X, z, lp, Xp = locs[:n], np.asfortranarray(X[:n]), np.asfortranarray(z[:n]), lp[:mp], np.asfortranarray(Xp[:mp])
    with pytest.raises(Exception):
        ca.cocoPredict_vecchia_joint(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, 71)
    got = ca.cocoPredict_vecchia_joint(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, 63)
    mean = ca.cocoSim_cond_vecchia(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, np.zeros((mp, 1)), 63)
    assert got["mean"].shape == (mp,) and got["cov"].shape == (mp, mp)
    assert np.array_equal(got["mean"], mean[:, 0])
    sym = _rel(got["cov"], got["cov"].T)
    some = ca.cocoPredict_vecchia_joint(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, 63, cov_idx=[12, 3])
    assert np.array_equal(some["cov"], got["cov"][:, [11, 2]])
    no = 40
    full = ca.cocoPredict_vecchia_joint(th, locs[:no], lp, X[:no], Xp, wl.SMOOTH_LIMITS, z[:no], no + mp - 1)
    S = O.cov_rns(th, np.vstack([locs[:no], lp]), np.vstack([X[:no], Xp]), wl.SMOOTH_LIMITS)
    want = S[no:, no:] - S[no:, :no] @ np.linalg.solve(S[:no, :no], S[no:, :no].T)
    resid = z[:no, 0] - X[:no] @ th["mean"]
    want_mean = Xp @ th["mean"] + S[no:, :no] @ np.linalg.solve(S[:no, :no], resid)
    errs = (sym, _rel(full["cov"], want), _rel(full["mean"], want_mean))
    _report("joint prediction: symmetry, dense conditional covariance and mean", "n60 / n40 mp12", max(errs))
    assert max(errs) < PARITY, errs
