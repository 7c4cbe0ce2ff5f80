"""U^-1 on a Vecchia fit on the GPU (cocons_vecchia_unwhiten, cocons_sim_vecchia, cocons_vecchia_schedule) against
tests/vecchia_sim_reference.py on the oracle's matrices, on the problem of test_gpu_dense_sizes.problem and the tables of
test_gpu_vecchia.table.

Bound of every comparison with a reference: the project's parity bound, PARITY = 1e-8 of test_gpu_dense_sizes, relative to the
largest magnitude of the compared array.  (On these cases the reference recursion in double differs from long double by at
most 3.1e-15 and by at most 9.6e-16 under a reversed order of summation, and cond(U) <= 64: the bound leaves seven orders for
the device's own rounding and hides nothing.)  Schedules are compared as integers, bits with np.array_equal.  Every test
prints its worst error on one line that starts with `vecchia-sim-report`; the measured figures stand in
tests/golden/VECCHIA_SIM_REPORT.md."""
import contextlib
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_reference as VR  # noqa: E402
import vecchia_sim_reference as VS  # noqa: E402
from test_gpu_dense_sizes import PARITY, problem  # noqa: E402
from test_gpu_vecchia import MS, SIZES, _duplicate_site, _fit, _theta, table  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCH = "COCONS_VECCHIA_SIM_FUSE"


def _report(what, case, err):
    print("vecchia-sim-report gpu | %s | %s | %.2e" % (what, case, err))


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
def columns(n, c=3):
    W = np.asfortranarray(np.random.default_rng(1000 + n).standard_normal((n, c)))
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def special(kind):
    """n = 641.  chain: row i names i - 1 (depth 641).  zero: nobody names anybody (depth 1).  wide: rows 2 .. 64 a chain and
    every later row names row 1 only -- one level of 578 rows (row 2 and the 577 late rows) next to 63 levels of one row, so
    both launch kinds and the switch between them run."""
    n = 641
    nn = np.zeros((n, 1 if kind == "chain" else 3), dtype=np.int32, order="F")
    if kind == "chain":
        nn[1:, 0] = np.arange(1, n)
    elif kind == "wide":
        nn[1:64, 0] = np.arange(1, 64)
        nn[64:, 0] = 1
    nn.setflags(write=False)
    return nn


def _table_of(spec):
    return special(spec) if isinstance(spec, str) else table(*spec)


@functools.lru_cache(maxsize=None)
def reference(spec):
    nn = _table_of(spec)
    n = nn.shape[0]
    x = VS.unwhiten(problem(n)[6], nn, columns(n))
    x.setflags(write=False)
    return x


def _spec_fit(spec):
    nn = _table_of(spec)
    return _fit(nn.shape[0], nn.shape[1], nn=nn)


def _check_unwhiten(spec, case):
    n = _table_of(spec).shape[0]
    th, W = problem(n)[2], columns(n)
    f = _spec_fit(spec)
    try:
        x = f.unwhiten_core(th, W)
        back = f.whiten_core(th, x)[0]
    finally:
        f.close()
    errs = (_rel(x, reference(spec)), _rel(back, W))
    _report("unwhiten, whiten(unwhiten(W))", case, max(errs))
    assert max(errs) < PARITY, errs


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_unwhiten_parity_and_round_trip(n, m):
    """rows with fewer than m predecessors, the full 64-row block (m = 63), the 64 / 65 seam"""
    _check_unwhiten((n, m), "n%d m%d" % (n, m))


@pytest.mark.parametrize("n,m", ((65, 10), (300, 30)))
def test_tables_with_zeros_inside_rows_and_an_empty_row(n, m):
    _check_unwhiten((n, m, True), "holes n%d m%d" % (n, m))


@pytest.mark.parametrize("kind", ("chain", "zero", "wide"))
def test_tables_of_known_shape(kind):
    """a chain (fused runs only), independent rows (one wide level), and a wide level between narrow ones (both launch kinds)"""
    _check_unwhiten(kind, "%s n641" % kind)


SCHEDULES = [(n, m) for n in SIZES for m in MS] + [(65, 10, True), (300, 30, True), "chain", "zero", "wide"]


@pytest.mark.parametrize("spec", SCHEDULES, ids=str)
def test_schedules_equal_the_reference_exactly(spec):
    nn = _table_of(spec)
    n = nn.shape[0]
    f = _spec_fit(spec)
    try:
        for n_fixed in sorted({0, 64, n - 1}):
            if not 0 <= n_fixed < n:
                continue
            want = VS.levels(nn, n_fixed)
            got = f.schedule(n_fixed)
            assert got["levels"].dtype == np.int32 and np.array_equal(got["levels"], want), (spec, n_fixed)
            assert got["depth"] == int(want.max())
            assert got["widest"] == int(np.bincount(want[n_fixed:]).max())
            assert 1 <= got["launches"] <= got["depth"]
            with _switch("0"):
                assert f.schedule(n_fixed)["launches"] == got["depth"]         # one launch per level
        if spec == "chain":
            assert f.schedule(0)["depth"] == 641 and f.schedule(0)["launches"] == 1
        if spec == "zero":
            assert f.schedule(0)["depth"] == 1 and f.schedule(0)["widest"] == 641
        if spec == "wide":
            # one column: level 1 (one row) fused, level 2 (578 rows: above the 256 (row, column) pairs a fused level may
            # have) on its own, levels 3 .. 64 (one row each) fused
            s = f.schedule(0)
            assert (s["depth"], s["widest"], s["launches"]) == (64, 578, 3)
    finally:
        f.close()
    _report("schedule: levels, depth, widest", str(spec), 0.0)


@pytest.mark.parametrize("spec", ((641, 30), (65, 63), "wide", "chain"), ids=str)
def test_bits_repeat_columns_and_the_fuse_switch(spec):
    n = _table_of(spec).shape[0]
    th, W = problem(n)[2], columns(n)
    f = _spec_fit(spec)
    try:
        a, b = f.unwhiten_core(th, W), f.unwhiten_core(th, W)
        cols = [f.unwhiten_core(th, W[:, k]) for k in range(3)]
        with _switch("0"):
            launches = f.schedule()["launches"]
            c = f.unwhiten_core(th, W)
        g = _spec_fit(spec)
        try:
            with _switch("0"):
                d = g.unwhiten_core(th, W)                  # a handle that never saw the default
        finally:
            g.close()
        depth = f.schedule()["depth"]
    finally:
        f.close()
    assert launches == depth
    _report("bits: repeat, columns, fuse off", str(spec), float(np.max(np.abs(a - c))))
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    for k in range(3):
        assert np.array_equal(cols[k][:, 0], a[:, k])


def test_exact_with_all_predecessors():
    """n = 64, m = 63, every predecessor: U^-1 is the Cholesky factor of Sigma -- cocons_sim_dense's fields, and numpy's"""
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
    E = rng.standard_normal((n, 3))
    S = O.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
    want = (X @ th["mean"])[:, None] + np.linalg.cholesky(S) @ E
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    d = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        got, dense = f.sim_core(th, E), d.sim_core(th, E)
        host = ca.cocoSim_vecchia(th, locs, X, wl.SMOOTH_LIMITS, E, fit=f)
    finally:
        f.close()
        d.close()
    errs = (_rel(got, dense), _rel(got, want))
    _report("exact: dense handle and numpy", "n64 m63", max(errs))
    assert max(errs) < PARITY, errs
    assert np.array_equal(host, got)


@pytest.mark.parametrize("nu", (0.5, 1.5, 2.5))
def test_closed_form_modes(nu):
    """a fixed smoothness (smooth.limits equal, a zero smooth vector): the closed forms the dense assembly would choose"""
    from oracle import oracle as O
    n, m = 300, 30
    locs, X, th0, z = problem(n)[:4]
    th = OrderedDict((k, np.array(v, copy=True)) for k, v in th0.items())
    th["smooth"] = np.zeros(3)
    S = O.cov_rns(th, locs, X, (nu, nu))
    want = VS.unwhiten(S, table(n, m), columns(n))
    f = _fit(n, m, smooth_limits=(nu, nu))
    try:
        got = f.unwhiten_core(th, columns(n))
    finally:
        f.close()
    err = _rel(got, want)
    _report("closed forms", "nu%.1f n%d m%d" % (nu, n, m), err)
    assert err < PARITY, err


@functools.lru_cache(maxsize=None)
def joint(m, ordered):
    """problem(65)'s observations followed by its 70 new locations.  ordered: the m nearest earlier rows of the joint set (new
    rows name earlier new rows).  Otherwise the observations keep table(65, m) and every new row names its m nearest
    observations (vecchia_neighbours_pred)."""
    from cocons_amd import host
    locs, X, th, z, lp, Xp = problem(65)[:6]
    la, Xa = np.vstack([locs, lp]), np.asfortranarray(np.vstack([X, Xp]))
    za = np.asfortranarray(np.vstack([z, np.full((lp.shape[0], z.shape[1]), 1e3)]))       # the new rows' z is never read
    if ordered:
        nn = host.vecchia_neighbours(la, m)
        assert np.any(nn[65:] > 65)
    else:
        nn = np.asfortranarray(np.vstack([table(65, m), host.vecchia_neighbours_pred(locs, lp, m)]))
    for a in (la, Xa, za, nn):
        a.setflags(write=False)
    return la, Xa, za, nn


def test_conditional_mean_equals_local_kriging_when_new_rows_name_observations_only():
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    m = 10
    locs, X, th, z, lp, Xp = problem(65)[:6]
    d = np.hypot(lp[:, None, 0] - locs[None, :, 0], lp[:, None, 1] - locs[None, :, 1])
    assert d.min() > 0.01                                   # the new sites are distinct from the observations
    la, Xa, za, nn = joint(m, False)
    mp = lp.shape[0]
    f = ca.CoconsVecchiaFit(la, Xa, za, wl.SMOOTH_LIMITS, nn)
    o = _fit(65, m)
    try:
        got = f.sim_core(th, np.zeros((mp, 1)), n_fixed=65, z_col=1)
        st = o.predict_core(th, lp, Xp, host.vecchia_neighbours_pred(locs, lp, m), z_col=1)[0]
    finally:
        f.close()
        o.close()
    want = Xp @ th["mean"] + st
    err = _rel(got[:, 0], want)
    _report("conditional mean against predict_core", "n65 mp%d m%d" % (mp, m), err)
    assert err < PARITY, err


def test_conditional_draw_equals_the_reference_recursion_on_the_ordered_joint_table():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    m = 10
    locs, X, th, z, lp, Xp = problem(65)[:6]
    la, Xa, za, nn = joint(m, True)
    mp = lp.shape[0]
    E = np.random.default_rng(77).standard_normal((mp, 2))
    S = O.cov_rns(th, la, Xa, wl.SMOOTH_LIMITS)
    resid = z[:, 1] - X @ th["mean"]
    x = VS.unwhiten(S, nn, E, n_fixed=65, x_fixed=np.column_stack([resid, resid]))
    want = (Xp @ th["mean"])[:, None] + x[65:]
    f = ca.CoconsVecchiaFit(la, Xa, za, wl.SMOOTH_LIMITS, nn)
    try:
        got = f.sim_core(th, E, n_fixed=65, z_col=1)
        mean_only = f.sim_core(th, np.zeros((mp, 1)), n_fixed=65, z_col=1)
    finally:
        f.close()
    x0 = VS.unwhiten(S, nn, np.zeros((mp, 1)), n_fixed=65, x_fixed=resid[:, None])
    errs = (_rel(got, want), _rel(mean_only[:, 0], Xp @ th["mean"] + x0[65:, 0]))
    _report("conditional draw and mean, ordered joint table", "n65 mp%d m%d" % (mp, m), max(errs))
    assert max(errs) < PARITY, errs


def test_host_conditional_function_builds_the_joint_handle_on_the_device():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    m = 10
    locs, X, th, z, lp, Xp = problem(65)[:6]
    la, Xa, za = joint(m, True)[:3]
    E = np.random.default_rng(78).standard_normal((lp.shape[0], 2))
    f = ca.CoconsVecchiaFit.from_knn(la, Xa, za, wl.SMOOTH_LIMITS, m)
    try:
        want = f.sim_core(th, E, n_fixed=65)
    finally:
        f.close()
    got = ca.cocoSim_cond_vecchia(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, E, m)
    assert np.array_equal(got, want)


def _raw_unwhiten(f, th, W):
    from cocons_amd import host
    out = np.full(W.shape, 7.0, order="F")
    T = host.theta_table(th)
    return f._L.cocons_vecchia_unwhiten(f._h, host._p(T), W.shape[1], host._p(np.asfortranarray(W)), host._p(out)), out


def test_failing_block_returns_its_row_and_leaves_the_handle_usable():
    """test_gpu_vecchia's failing block: row 58 on the coordinates of row 41 and conditioned on it alone, so the block is
    [[a, a], [a, b]] with a, b the two sites' variances and the sign of the std.dev slopes decides its second pivot.  A
    numerical refusal, not a device fault."""
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    locs, X, th0, z, nn = _duplicate_site(False)
    slope = np.array([0.0, 0.3, -0.2])
    up = float((X[57] - X[40]) @ slope) > 0                # b > a with these slopes
    good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
    W = columns(65)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    g = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        fresh = g.unwhiten_core(good, W)
        rc, out = _raw_unwhiten(f, bad, W)
        assert rc == 58 and np.all(out == 7.0)
        with pytest.raises(_lib.CholeskyError) as e:
            f.sim_core(bad, W)
        assert e.value.minor == 58
        # the rows in front of it fixed: still the first block that is factored
        E, o = np.zeros(8), np.full(8, 7.0)
        T, mean = host.theta_table(bad), np.ascontiguousarray(bad["mean"])
        assert f._L.cocons_sim_vecchia(f._h, host._p(T), host._p(mean), 57, 0, 1, host._p(E), host._p(o)) == 58
        assert np.all(o == 7.0)
        assert np.array_equal(f.unwhiten_core(good, W), fresh)
    finally:
        f.close()
        g.close()
    _report("failing block", "n65 row 58", 0.0)


def test_new_entries_between_the_others_keep_every_result_at_its_fresh_handle_bits():
    """value, gradient, information, whiten and predict share V->aos, V->B and V->W with the new entries"""
    from cocons_amd import host
    n, m = 300, 30
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    W = columns(n)
    nnp = host.vecchia_neighbours_pred(locs, lp, m)
    dirs = np.eye(18)[:4]

    def others(f):
        return [np.concatenate([[f.neg2loglik_core(th)[0]], f.neg2loglik_core(th)[1]]),
                np.concatenate([a.ravel() for a in f.neg2loglik_grad_core(th)[1:]]),
                np.concatenate([a.ravel() for a in f.fisher_core(th, dirs)]),
                np.concatenate([a.ravel() for a in f.whiten_core(th, Rz)]),
                np.concatenate(f.predict_core(th, lp, Xp, nnp))]

    def new(f):
        return [f.unwhiten_core(th, W), f.sim_core(th, W[:, :2]), f.sim_core(th, W[64:, :1], n_fixed=64, z_col=1),
                f.schedule(64)["levels"], f.schedule()["levels"]]

    a, b, c = _fit(n, m), _fit(n, m), _fit(n, m)
    try:
        fresh_others, fresh_new = others(a), new(b)
        mixed_new = new(c)
        mixed_others = others(c)
        again_new = new(c)
        interleaved = []
        for k in range(5):
            interleaved.append(others(c)[k])
            c.unwhiten_core(th, W[:, :1])
    finally:
        for f in (a, b, c):
            f.close()
    for got in (mixed_new, again_new):
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh_new))
    for got in (mixed_others, interleaved):
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh_others))
    _report("order of calls", "n%d m%d" % (n, m), 0.0)


def test_refusals_that_need_a_handle_and_the_bytes_of_the_handle():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n = 65
    locs, X, th, z = problem(n)[:4]
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    W, out = np.asfortranarray(columns(n)), np.full((n, 3), 7.0, order="F")
    out4 = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    vec = _fit(n, 10)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        L = vec._L
        for n_fixed in (n, n + 5):
            assert L.cocons_sim_vecchia(vec._h, host._p(T), host._p(mean), n_fixed, 0, 3, host._p(W), host._p(out)) == -1
            assert _lib.last_error() == "cocons_sim_vecchia: n_fixed = %d is outside 0 .. 64" % n_fixed
            assert L.cocons_vecchia_schedule(vec._h, n_fixed, None, out4) == -1
            assert _lib.last_error() == "cocons_vecchia_schedule: n_fixed = %d is outside 0 .. 64" % n_fixed
        assert L.cocons_sim_vecchia(vec._h, host._p(T), host._p(mean), 0, 2, 3, host._p(W), host._p(out)) == -1
        assert _lib.last_error() == "cocons_sim_vecchia: z_col = 2 is outside 0 .. 1"
        assert L.cocons_vecchia_unwhiten(dense._h, host._p(T), 3, host._p(W), host._p(out)) == -1
        assert _lib.last_error().startswith("cocons_vecchia_unwhiten: not a Vecchia fit")
        assert L.cocons_sim_vecchia(dense._h, host._p(T), host._p(mean), 0, 0, 3, host._p(W), host._p(out)) == -1
        assert _lib.last_error().startswith("cocons_sim_vecchia: not a Vecchia fit")
        assert L.cocons_vecchia_schedule(dense._h, 0, None, out4) == -1
        assert _lib.last_error().startswith("cocons_vecchia_schedule: not a Vecchia fit")
        assert np.all(out == 7.0) and list(out4) == [-7] * 4
        # the schedule and the coefficients are the handle's and are counted
        before = vec.info()["bytes"]
        vec.unwhiten_core(th, W)
        s = vec.schedule()
        assert vec.info()["bytes"] - before >= n * 11 * 8 and s["bytes"] >= n * 11 * 8
    finally:
        vec.close()
        dense.close()
