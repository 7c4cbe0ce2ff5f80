"""cocoSim's sparse branch (R/sim.R:177-217) on the device: cocons_sim_taper / CoconsTaperFit.sim_core against a numpy
restatement -- S = taper o cov_rns_taper (CPU oracle), L_P = chol(S[o, o]), fields[o] = L_P E + trend[o] -- for the
handle's own order (band_trmm_kernel on the packed band and on the dense buffer), for a caller's pivot (the twin
handle), the order-free identity, a scale check through an independent solve, refusals, and the R glue."""
import numpy as np
import pytest

from test_gpu_parity import _problem, _taper_pattern

pytestmark = pytest.mark.gpu

TOL = 1e-10          # max abs error over max abs value


def _delta(n):
    return 0.25 if n < 1000 else (0.12 if n < 3000 else 0.06)      # as test_taper_objective_vs_oracle


def _S(oracle, th, locs, X, ref_taper):
    from cocons_amd import workloads as wl
    ci, rp, ent = ref_taper
    n = locs.shape[0]
    vals = ent * oracle.cov_rns_taper(th, locs, X, ci, rp, wl.SMOOTH_LIMITS)
    S = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    S[rows, ci - 1] = vals
    return S


def _want(S, order, E, trend):
    o = np.asarray(order) - 1
    Lp = np.linalg.cholesky(S[np.ix_(o, o)])
    out = np.empty_like(E)
    out[o] = Lp @ E + trend[o, None]
    return out


def _close(got, want):
    return float(np.max(np.abs(got - want))) <= TOL * float(np.max(np.abs(want)))


def _setup(n, r=1, seed=0):
    locs, X, th, rng = _problem(n, seed=seed)
    th["mean"] = np.array([0.3, -0.2, 0.1])
    z = rng.standard_normal((n, r))
    return locs, X, th, z, rng


@pytest.mark.parametrize("n", [150, 1500, 4000])
def test_fast_route_own_order(oracle, n):
    """pivot = NULL: the handle's RCM order (packed band at n = 4000), 1, 7, 64 and 100 draws (a partial block, one
    block, a block and a part)."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, rng = _setup(n, seed=800 + n)
    ref_taper = _taper_pattern(locs, _delta(n))
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
    try:
        order = fit.order()
        assert sorted(order.tolist()) == list(range(1, n + 1))
        S = _S(oracle, th, locs, X, ref_taper)
        trend = X @ th["mean"]
        for nsim in (1, 7, 64, 100):
            E = rng.standard_normal((n, nsim))
            got = fit.sim_core(th, E)
            assert got.shape == (n, nsim)
            assert _close(got, _want(S, order, E, trend)), nsim
    finally:
        fit.close()


def test_dense_buffer_and_dense_factorisation(oracle, monkeypatch):
    """The same product from the dense buffer (COCONS_TAPER_PACKED=0) and without an envelope (COCONS_TAPER_BAND=0)."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 4000
    locs, X, th, z, rng = _setup(n, seed=4100)
    ref_taper = _taper_pattern(locs, 0.06)
    S = _S(oracle, th, locs, X, ref_taper)
    trend = X @ th["mean"]
    E = rng.standard_normal((n, 70))
    for var in ("COCONS_TAPER_PACKED", "COCONS_TAPER_BAND"):
        monkeypatch.setenv(var, "0")
        fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
        try:
            assert _close(fit.sim_core(th, E), _want(S, fit.order(), E, trend)), var
        finally:
            fit.close()
        monkeypatch.delenv(var)


def test_draw_equal_route_pivot(oracle):
    """A caller's pivot (random, reversed): the factor of S[pivot, pivot] -- the twin handle, reused while the pivot
    stays; pivot = the handle's own order is the fast route bit for bit; two calls are bit-identical."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 700
    locs, X, th, z, rng = _setup(n, seed=7000)
    ref_taper = _taper_pattern(locs, 0.25)
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
    try:
        S = _S(oracle, th, locs, X, ref_taper)
        trend = X @ th["mean"]
        E = rng.standard_normal((n, 65))
        rnd = (rng.permutation(n) + 1).astype(np.int32)
        rev = np.arange(n, 0, -1, dtype=np.int32)
        for piv in (rnd, rev, rnd):
            got = fit.sim_core(th, E, pivot=piv)
            assert _close(got, _want(S, piv, E, trend))
            assert np.array_equal(got, fit.sim_core(th, E, pivot=piv))
        own = fit.sim_core(th, E)
        assert np.array_equal(own, fit.sim_core(th, E, pivot=fit.order()))
        assert np.array_equal(own, fit.sim_core(th, E))
        assert not np.array_equal(own, fit.sim_core(th, E, pivot=rev))
    finally:
        fit.close()


def test_order_free_identity(oracle):
    """E = I (nsim = n): (Y - trend)(Y - trend)' = S whatever the order."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 400
    locs, X, th, z, rng = _setup(n, seed=400)
    ref_taper = _taper_pattern(locs, 0.25)
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
    try:
        S = _S(oracle, th, locs, X, ref_taper)
        D = fit.sim_core(th, np.eye(n)) - (X @ th["mean"])[:, None]
        assert np.max(np.abs(D @ D.T - S)) <= 1e-12 * np.max(np.abs(S))
        D = fit.sim_core(th, np.eye(n), pivot=(rng.permutation(n) + 1)) - (X @ th["mean"])[:, None]
        assert np.max(np.abs(D @ D.T - S)) <= 1e-12 * np.max(np.abs(S))
    finally:
        fit.close()


def _grid_pattern(locs, delta):
    """Wendland-1 taper of range delta, 1-based CSR, by cells of edge delta (tools/taper_timing.py's builder)."""
    cell = {}
    for i, (x, y) in enumerate(locs):
        cell.setdefault((int(x / delta), int(y / delta)), []).append(i)
    ci, rp, ent = [], [1], []
    for i, (x, y) in enumerate(locs):
        cx, cy = int(x / delta), int(y / delta)
        cand = np.array(sorted(j for a in (-1, 0, 1) for b in (-1, 0, 1) for j in cell.get((cx + a, cy + b), [])))
        d = np.sqrt(np.sum((locs[cand] - locs[i]) ** 2, axis=1))
        keep = d <= delta
        h = d[keep] / delta
        ci.extend((cand[keep] + 1).tolist())
        ent.extend(((1 - h) ** 4 * (4 * h + 1)).tolist())
        rp.append(len(ci) + 1)
    return np.array(ci, dtype=np.int32), np.array(rp, dtype=np.int32), np.array(ent)


def test_scale_n40000_through_an_independent_solve():
    """n = 40 000 (200 x 200 grid, packed band), 8 draws: a second taper handle with z = Y - trend and mean 0 returns
    the quadratic forms (L e)' S^-1 (L e) = ||e||^2; the simulating handle's objective is unchanged afterwards."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    g = 200
    n = g * g
    locs = wl.grid_locs(g)
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full(scale0=np.log(0.05))
    th["mean"] = np.array([0.3, -0.2, 0.1])
    ref_taper = _grid_pattern(locs, 0.03)
    rng = np.random.default_rng(40000)
    z = rng.standard_normal((n, 1))
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
    try:
        v0, p0 = fit.neg2loglik_core(th)
        E = rng.standard_normal((n, 8))
        Y = fit.sim_core(th, E)
        assert np.all(np.isfinite(Y))
        v1, p1 = fit.neg2loglik_core(th)
        assert v1 == v0 and np.array_equal(p1, p0)
    finally:
        fit.close()
    th0 = dict(th)
    th0["mean"] = np.zeros(3)
    chk = ca.CoconsTaperFit(locs, X, Y - (X @ th["mean"])[:, None], wl.SMOOTH_LIMITS, *ref_taper)
    try:
        _, parts = chk.neg2loglik_core(th0)
        want = np.sum(E * E, axis=0)
        assert np.max(np.abs(np.asarray(parts[1:9]) - want) / want) <= 1e-9
    finally:
        chk.close()


def test_refusals_and_recovery(oracle):
    """A dense handle, a pivot that is not a permutation, a theta that makes S not positive definite: refused (status
    k > 0 for the last), and the handle's next valid call is exactly what it was before."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 4000
    locs, X, th, z, rng = _setup(n, seed=4200)
    ref_taper = _taper_pattern(locs, 0.06)
    dense = ca.CoconsFit(locs[:300], X[:300], z[:300], wl.SMOOTH_LIMITS)
    try:
        with pytest.raises(ca.CoconsHipError, match="taper"):
            ca.CoconsTaperFit.sim_core(dense, th, rng.standard_normal((300, 2)))
    finally:
        dense.close()
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
    try:
        E = rng.standard_normal((n, 9))
        first = fit.sim_core(th, E)
        for bad in (0, n + 1, "dup"):
            piv = np.arange(1, n + 1, dtype=np.int32)
            if bad == "dup":
                piv[5] = piv[6]
            else:
                piv[17] = bad
            with pytest.raises(ca.CoconsHipError, match="permutation"):
                fit.sim_core(th, E, pivot=piv)
            assert np.array_equal(fit.sim_core(th, E), first)
        th_bad = {k: np.array(v, dtype=float).copy() for k, v in th.items()}
        th_bad["std.dev"][0] = -np.inf
        th_bad["nugget"][0] = -np.inf
        with pytest.raises(ca.CholeskyError) as ei:
            fit.sim_core(th_bad, E)
        assert ei.value.minor > 0
        assert np.array_equal(fit.sim_core(th, E), first)
        S = _S(oracle, th, locs, X, ref_taper)
        assert _close(first, _want(S, fit.order(), E, X @ th["mean"]))
    finally:
        fit.close()


def test_glue_sim_taper_matches_sim_core():
    """`_cocons_hip_sim_taper` through the R stub: R NULL pivot and an integer pivot, bit for bit sim_core's fields."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from test_glue_exec import RStub
    R = RStub()
    n = 700
    locs, X, th, z, rng = _setup(n, seed=7100)
    ci, rp, ent = _taper_pattern(locs, 0.25)
    E = rng.standard_normal((n, 5))
    piv = (rng.permutation(n) + 1).astype(np.int32)
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, ent)
    try:
        want0, want1 = fit.sim_core(th, E), fit.sim_core(th, E, pivot=piv)
    finally:
        fit.close()
    h = R.call("_cocons_hip_fit_create_taper", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer(ci), R.integer(rp), R.real(ent))
    st, got0 = R.value(R.call("_cocons_hip_sim_taper", h, R.theta(th), R.real(th["mean"]), R.real(E), R.nil))
    assert int(st[0]) == 0 and np.array_equal(got0, want0)
    st, got1 = R.value(R.call("_cocons_hip_sim_taper", h, R.theta(th), R.real(th["mean"]), R.real(E), R.integer(piv)))
    assert int(st[0]) == 0 and np.array_equal(got1, want1)
    with pytest.raises(RuntimeError, match="pivot"):
        R.call("_cocons_hip_sim_taper", h, R.theta(th), R.real(th["mean"]), R.real(E), R.real(piv.astype(float)))
    R.L.stub_gc(0, None)
