"""cocons_fisher_vecchia on the GPU against tests/vecchia_fisher_reference.py, on the problems of
test_gpu_vecchia (test_gpu_dense_sizes.problem: uniform sites in no spatial order, two realisations, p = 3 from n = 3 on).

Bounds: TOL = 1e-7 in fisher_reference.metric against the numpy statement -- the project's tolerance for the same pair partials
(test_gpu_fisher.py) --, info_mean within 1e-10 of its largest entry, the scaling direction within 1e-9 n of r n / 2, and
1e-9 in the metric against cocons_fisher_dense where the table names every predecessor.  Every comparison prints its worst
error on a line that starts with `vecchia-fisher-report`; the measured figures stand in
tests/golden/VECCHIA_FISHER_REPORT.md."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
import vecchia_fisher_reference as VF  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402
from test_gpu_vecchia import SIZES, MS, table, pred_problem, _theta  # noqa: E402
from test_gpu_vecchia_grad import _coincident  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-7
MEAN_TOL = 1e-10
DENSE_TOL = 1e-9


def _report(what, case, err):
    print("vecchia-fisher-report gpu | %s | %s | %.2e" % (what, case, err))


def _limits(sl=None):
    from cocons_amd import workloads as wl
    return tuple(wl.SMOOTH_LIMITS) if sl is None else tuple(sl)


def _make(locs, X, z, nn, sl=None):
    import cocons_amd as ca
    return ca.CoconsVecchiaFit(locs, X, z, _limits(sl), nn)


def dirs19(p):
    """the 6 p unit tables, then the scaling direction: 19 at p = 3"""
    return np.concatenate([np.eye(6 * p).reshape(6 * p, 6, p), FR.scaling_direction(p)[None]])


def mixes(nd, p=3):
    """the scaling direction, then seeded random mixes over all families"""
    return np.concatenate([FR.scaling_direction(p)[None], np.random.default_rng(41).standard_normal((nd - 1, 6, p))])


@functools.lru_cache(maxsize=None)
def _matrices(n):
    """(Sigma, Sigma_a) of problem(n) for dirs19, computed once and left unchanged"""
    from cocons_amd import host
    locs, X, th = problem(n)[:3]
    S, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, _limits(), dirs19(X.shape[1]))
    S.setflags(write=False)
    Sa.setflags(write=False)
    return S, Sa


@functools.lru_cache(maxsize=None)
def reference(n, m, holes=False):
    S, Sa = _matrices(n)
    out = VF.info_last_row(S, Sa, table(n, m, holes), problem(n)[3].shape[1], np.asarray(problem(n)[1]))
    for a in out:
        a.setflags(write=False)
    return out


def _check(got, want, case, n=None, r=None, scaling=None):
    info, im = got
    errs = (FR.metric(info, want[0]), float(np.max(np.abs(im - want[1])) / np.max(np.abs(want[1]))))
    _report("info (metric)", case, errs[0])
    _report("info_mean (relative)", case, errs[1])
    assert np.array_equal(info, info.T) and np.array_equal(im, im.T), case
    assert errs[0] <= TOL and errs[1] <= MEAN_TOL, (case, errs)
    if scaling is not None:
        gap = abs(info[scaling, scaling] - r * n / 2)
        _report("I(v_s, v_s) - r n / 2, over n", case, gap / n)
        assert gap <= 1e-9 * n, (case, gap)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n, m):
    """rows with fewer than m predecessors, a full 64-row block (m = 63), the 64 / 65 seam, pair walks of one pass and of many;
    19 directions at p = 3: two groups"""
    locs, X, th, z = problem(n)[:4]
    p = X.shape[1]
    f = _make(locs, X, z, table(n, m))
    try:
        got = f.fisher_core(th, dirs19(p))
    finally:
        f.close()
    _check(got, reference(n, m), "n%d m%d ndir%d" % (n, m, 6 * p + 1), n, z.shape[1], 6 * p)


@pytest.mark.parametrize("ndir", (1, 7, 17, 19))
def test_numbers_of_directions(ndir):
    """one direction, a partly filled group, one more than a group, and the unit tables with the scaling direction"""
    from cocons_amd import host
    n, m = 300, 30
    locs, X, th, z = problem(n)[:4]
    D = dirs19(3) if ndir == 19 else mixes(ndir)
    want = reference(n, m) if ndir == 19 else VF.statement(host.theta_table(th), locs, X, _limits(), D, table(n, m), z.shape[1])
    f = _make(locs, X, z, table(n, m))
    try:
        got = f.fisher_core(th, D)
    finally:
        f.close()
    _check(got, want, "n%d m%d ndir%d" % (n, m, ndir), n, z.shape[1], 18 if ndir == 19 else 0)


@pytest.mark.parametrize("n,m", ((65, 10), (300, 30)))
def test_tables_with_holes_and_unsorted_rows_and_a_row_without_neighbours(n, m):
    locs, X, th, z = problem(n)[:4]
    nn = np.array(table(n, m, True), order="F")
    rng = np.random.default_rng(n)
    for i in range(n):
        nn[i] = nn[i, rng.permutation(m)]              # zeros anywhere, the neighbours in no order
    assert np.any(np.diff(nn[n - 1][nn[n - 1] > 0]) < 0) and np.all(nn[n // 2] == 0)
    f = _make(locs, X, z, nn)
    try:
        got = f.fisher_core(th, dirs19(3))
    finally:
        f.close()
    _check(got, reference(n, m, True), "holes, unsorted n%d m%d" % (n, m), n, z.shape[1], 18)


@pytest.mark.parametrize("nu,slopes", ((0.5, False), (1.5, False), (2.5, False), (1.0, True)))
def test_closed_forms_and_the_bessel_branch_at_a_fixed_smoothness(nu, slopes):
    """smooth.limits equal: with a zero smooth vector the three closed forms; with slopes in it the Bessel branch at a
    smoothness that is the same everywhere.  The free smoothness is every other test here."""
    from cocons_amd import host
    import grad_reference as GR
    n, m = 300, 30
    locs, X, th0, z = problem(n)[:4]
    th = _theta(th0) if slopes else _theta(th0, smooth=np.zeros(3))
    want_mode = "geom" if slopes else {0.5: "half", 1.5: "threehalf", 2.5: "fivehalf"}[nu]
    assert GR.select_mode(host.theta_table(th), (nu, nu))[0] == want_mode
    D = mixes(7)
    want = VF.statement(host.theta_table(th), locs, X, (nu, nu), D, table(n, m), z.shape[1])
    f = _make(locs, X, z, table(n, m), (nu, nu))
    try:
        got = f.fisher_core(th, dirs19(3))
        mix = f.fisher_core(th, D)
    finally:
        f.close()
    case = "nu%.1f%s n%d m%d" % (nu, " bessel" if slopes else "", n, m)
    _check(mix, want, case, n, z.shape[1], 0)
    assert np.all(got[0][12:15] == 0.0) and np.all(got[0][:, 12:15] == 0.0)      # no smooth row at a fixed smoothness


def test_exact_with_all_predecessors_against_the_dense_entry():
    """n = 64, m = 63, every predecessor: cocons_fisher_dense's information"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(6464)
    n = 64
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = np.array([0.3, -0.15, 0.2])
    z = np.asfortranarray(rng.standard_normal((n, 2)))
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    f = _make(locs, X, z, VR.all_predecessors(n))
    try:
        want = dense.fisher_core(th, dirs19(3))
        got = f.fisher_core(th, dirs19(3))
    finally:
        dense.close()
        f.close()
    errs = (FR.metric(got[0], want[0]), float(np.max(np.abs(got[1] - want[1])) / np.max(np.abs(want[1]))))
    _report("exact: cocons_fisher_dense, info (metric)", "n64 m63", errs[0])
    _report("exact: cocons_fisher_dense, info_mean (relative)", "n64 m63", errs[1])
    assert errs[0] <= DENSE_TOL and errs[1] <= DENSE_TOL, errs


def test_a_coincident_pair_of_sites():
    from cocons_amd import host
    locs, X, th, z, nn = _coincident()
    want = VF.statement(host.theta_table(th), locs, X, _limits(), dirs19(3), nn, z.shape[1])
    f = _make(locs, X, z, nn)
    try:
        got = f.fisher_core(th, dirs19(3))
    finally:
        f.close()
    _check(got, want, "coincident pair n65 m10", 65, z.shape[1], 18)


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
    want = VF.statement(host.theta_table(th), locs, X, _limits(), dirs19(3), nn, z.shape[1])
    f = _make(locs, X, z, nn)
    try:
        got = f.fisher_core(th, dirs19(3))
    finally:
        f.close()
    _check(got, want, "far pair n65 m10", n, z.shape[1], 18)


def test_more_rows_than_one_chunk():
    """The smallest n that runs in two chunks at ndir = 2 (chunks of 32768 rows): nu = 1/2, m = 10, against the statement
    segment by segment.  The same two directions among 19 run in chunks of 8192 rows and must give the same bits: the result
    does not depend on the chunking."""
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    n, m = 32769, 10
    rng = np.random.default_rng(33)
    locs = np.column_stack([np.sort(rng.uniform(0, 40, size=n)), rng.uniform(0, 0.2, size=n)])      # neighbours in x
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    z = rng.standard_normal((n, 1))
    th = _theta(wl.theta_full(scale0=np.log(0.2)), smooth=np.zeros(3), mean=[0.3, -0.15, 0.2])
    D = mixes(19)
    want = VF.statement_banded(host.theta_table(th), locs, X, (0.5, 0.5), D[:2], m)
    f = ca.CoconsVecchiaFit(locs, X, z, (0.5, 0.5), VF.banded_table(n, m))
    try:
        got = f.fisher_core(th, D[:2])
        again = f.fisher_core(th, D[:2])
        wide = f.fisher_core(th, D)
    finally:
        f.close()
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    assert np.array_equal(wide[0][:2, :2], got[0]) and np.array_equal(wide[1], got[1])
    _check(got, want, "n%d m%d nu0.5 ndir2 (two chunks)" % (n, m), n, 1, 0)


def _outputs(n, m, sort):
    locs, X, th, z = problem(n)[:4]
    old = os.environ.get("COCONS_SPATIAL_SORT")
    os.environ["COCONS_SPATIAL_SORT"] = sort
    try:
        f = _make(locs, X, z, table(n, m))
        try:
            out = f.fisher_core(th, dirs19(3))
        finally:
            f.close()
    finally:
        if old is None:
            os.environ.pop("COCONS_SPATIAL_SORT", None)
        else:
            os.environ["COCONS_SPATIAL_SORT"] = old
    return np.concatenate([out[0].ravel(), out[1].ravel()])


@pytest.mark.parametrize("n", (65, 641))
def test_bits_repeat_and_do_not_see_the_spatial_sort(n):
    a, b, c = _outputs(n, 30, "1"), _outputs(n, 30, "1"), _outputs(n, 30, "0")
    _report("bits: repeat, sort off", "n%d m30" % n, float(np.max(np.abs(a - c))))
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_bits_do_not_see_foreign_rows():
    """50 rows appended that name no neighbour and have a zero row of X: every weight of theirs is exactly zero, so both
    matrices keep their bits (a sum that ran over other rows' data, or in another order, would not)"""
    n, m, extra = 300, 30, 50
    locs, X, th, z = problem(n)[:4]
    rng = np.random.default_rng(9)
    locs2 = np.vstack([locs, rng.uniform(0, 1, size=(extra, 2))])
    X2 = np.asfortranarray(np.vstack([X, np.zeros((extra, 3))]))
    nn2 = np.zeros((n + extra, m), dtype=np.int32, order="F")
    nn2[:n] = table(n, m)
    f, g = _make(locs, X, z, table(n, m)), _make(locs2, X2, np.zeros((n + extra, 2)), nn2)
    try:
        a, b = f.fisher_core(th, dirs19(3)), g.fisher_core(th, dirs19(3))
    finally:
        f.close()
        g.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sequences_on_one_handle():
    """the information between value, gradient, whiten and predict calls, in both orders: every output has the bits a fresh
    handle gives"""
    n, m = 300, 30
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    nnp = pred_problem(n, m)[1]
    calls = OrderedDict(
        fisher=lambda f: f.fisher_core(th, dirs19(3)), value=lambda f: f.neg2loglik_core(th),
        fisher7=lambda f: f.fisher_core(th, mixes(7)), grad=lambda f: f.neg2loglik_grad_core(th),
        whiten=lambda f: f.whiten_core(th, Rz), predict=lambda f: f.predict_core(th, lp, Xp, nnp))

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


def _raw(f, th, D, entry="cocons_fisher_vecchia"):
    from cocons_amd import host
    D = np.ascontiguousarray(np.asarray(D, dtype=float).reshape(-1, 6 * f.p))
    info, im = np.full(D.shape[0] ** 2, 7.0), np.full(f.p ** 2, 7.0)
    T = host.theta_table(th)
    if entry == "cocons_fisher_reml":
        rc = f._L.cocons_fisher_reml(f._h, host._p(T), D.shape[0], host._p(D), host._p(info))
    elif entry == "cocons_fisher_taper":
        rc = f._L.cocons_fisher_taper(f._h, host._p(T), D.shape[0], host._p(D), 0, None, 0, host._p(info), host._p(im))
    else:
        rc = getattr(f._L, entry)(f._h, host._p(T), D.shape[0], host._p(D), host._p(info), host._p(im))
    return rc, info, im


def test_a_failing_block_is_reported_and_the_outputs_left_alone():
    """the coincident pair with the slopes of std.dev turned round: the block of row 58 is not positive definite.  The row is
    returned, no output is touched, and the good theta keeps its bits."""
    locs, X, th, z, nn = _coincident()
    bad = _theta(th, std_dev=-th["std.dev"])
    f = _make(locs, X, z, nn)
    try:
        good = f.fisher_core(th, dirs19(3))
        rc, info, im = _raw(f, bad, dirs19(3))
        assert rc == 58 and np.all(info == 7.0) and np.all(im == 7.0)
        with pytest.raises(Exception):
            f.fisher_core(bad, dirs19(3))
        after = f.fisher_core(th, dirs19(3))
        assert np.array_equal(good[0], after[0]) and np.array_equal(good[1], after[1])
    finally:
        f.close()


def test_refusals_both_ways():
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    n = 65
    locs, X, th, z = problem(n)[:4]
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    vec = _make(locs, X, z, table(n, 10))
    try:
        rc, info, im = _raw(dense, th, dirs19(3))
        assert rc == -1 and np.all(info == 7.0) and np.all(im == 7.0)
        assert _lib.last_error() == "cocons_fisher_vecchia: not a Vecchia fit (cocons_fit_create_vecchia makes one)"
        D = dirs19(3).copy()
        D[4, 2, 1] = np.inf
        rc, info, im = _raw(vec, th, D)
        assert rc == -1 and np.all(info == 7.0) and np.all(im == 7.0)
        assert _lib.last_error().startswith("cocons_fisher_vecchia: direction 4 has a non-finite entry")
        for entry in ("cocons_fisher_dense", "cocons_fisher_reml", "cocons_fisher_taper"):
            rc, info, im = _raw(vec, th, dirs19(3), entry)
            assert rc == -1 and np.all(info == 7.0) and np.all(im == 7.0), entry
            assert _lib.last_error().startswith(entry + ": not available on a Vecchia fit"), _lib.last_error()
        info_only = np.full(19 * 19, 7.0)                # info_mean may be NULL
        from cocons_amd import host
        T, D = host.theta_table(th), np.ascontiguousarray(dirs19(3).reshape(19, 18))
        assert vec._L.cocons_fisher_vecchia(vec._h, host._p(T), 19, host._p(D), host._p(info_only), None) == 0
        assert np.array_equal(info_only.reshape(19, 19), vec.fisher_core(th, dirs19(3))[0])
    finally:
        dense.close()
        vec.close()


def test_the_handle_counts_what_the_call_allocated():
    """O(n) doubles and one chunk of records, on the first call only: the site derivatives in two layouts (4 doubles a site
    each, one of them padded to the handle's stride), the directions, the records, their first-stage sums and the totals"""
    n, m, nd, p = 641, 30, 19, 3
    locs, X, th, z = problem(n)[:4]
    f = _make(locs, X, z, table(n, m))
    try:
        before = f.info()["bytes"]
        f.fisher_core(th, dirs19(3))
        first = f.info()["bytes"]
        f.fisher_core(th, mixes(7))
        f.fisher_core(th, dirs19(3))
        assert f.info()["bytes"] == first
    finally:
        f.close()
    ncol = nd * (nd + 1) // 2 + p * (p + 1) // 2
    least = 8 * (4 * n + 4 * n + nd * 6 * p + n * ncol + ncol + ncol)
    _report("bytes added by the first call, over n", "n%d m%d ndir%d" % (n, m, nd), (first - before) / n)
    assert least <= first - before <= least + 8 * 4 * 512


def test_host_entry_against_the_statement():
    """getFisher_vecchia = J info J' + J_m info_mean J_m' of the numpy statement, every parameter free"""
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    n, m = 300, 30
    locs, X, th, z = problem(n)[:4]
    pp = OrderedDict((k, [True] * 3) for k in host.ASPECTS)
    par = wl.theta_vector_from_lists(th, pp)
    Jt, Jm = host.fisher_jacobian(par, pp)
    tl = ca.getModelLists(par, pp, "diff")
    I, Im = VF.statement(host.theta_table(tl), locs, X, _limits(), Jt.reshape(-1, 6, 3), table(n, m), z.shape[1])
    want = I + Jm @ Im @ Jm.T
    got = ca.getFisher_vecchia(par, pp, locs, X, wl.SMOOTH_LIMITS, z, n, table(n, m))
    gap = FR.metric(got, want)
    _report("getFisher_vecchia (metric)", "n%d m%d P%d" % (n, m, par.size), gap)
    assert got.shape == (par.size, par.size) and np.array_equal(got, got.T) and gap <= TOL
    ev = np.linalg.eigvalsh(got)
    assert ev[0] >= -1e-12 * ev[-1]
