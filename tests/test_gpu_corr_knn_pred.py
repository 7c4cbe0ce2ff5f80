"""cocons_vecchia_neighbours_corr_pred on the device against the numpy restatement of its rule
(host.vecchia_neighbours_corr_pred), integer for integer.  The restatement is fed by the rule's own wording: the device's
cocons_cov_rns_pred matrix of the new locations against the observations, the diagonals cocons_cov_rns_pred returns for the new
locations, and for the observations, predicted onto themselves, and the plain kNN tables of cocons_vecchia_neighbours with a
query set.  Sizes around the wavefront and several hundred rows on both sides, every width of the candidate table at which the
set in LDS changes its size, one and two hops, m = 1, m_cand and 63; a theta on the Bessel branch, one at a closed-form
smoothness (both with covariate-driven anisotropy) and one at a fixed smoothness that is no closed form -- the latter two make
the prediction branch's second set of records --; a lattice with exact ties, coincident observations, new sites on top of
observations and far outside the hull; repeated calls, calls at another width in between, what the handle keeps, and a rho
that is not finite."""
import ctypes

import numpy as np
import pytest

import corr_knn_reference as CR

pytestmark = pytest.mark.gpu

SHAPES = [(mc, hops) for mc in (1, 5, 30, 63) for hops in (1, 2)]
SIZES = [(1, 1), (2, 2), (64, 64), (65, 65), (700, 300), (1, 65), (65, 2), (700, 1), (64, 300)]        # (n, mp)


def _ms(mc, hops):
    cap = min(4032, mc + mc * mc * (hops - 1))
    return sorted(m for m in {1, mc, 63} if m <= cap)


def _thetas():
    from cocons_amd import workloads as wl
    closed = CR.theta_covariate()
    closed["smooth"] = np.zeros(3)
    return {"bessel": (CR.theta_covariate(), wl.SMOOTH_LIMITS), "closed": (closed, (1.5, 1.5)), "fixed": (closed, (0.8, 0.8))}


@pytest.fixture(scope="module")
def data():
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(20260407)
    locs = rng.uniform(0, 1, size=(700, 2))
    sc = wl.design_from_locs(locs)
    newlocs = rng.uniform(-0.05, 1.05, size=(300, 2))
    Xp = wl.design_from_locs(newlocs, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    out = (locs, np.asfortranarray(sc["std.covs"]), rng.standard_normal(700), newlocs, np.asfortranarray(Xp))
    for a in out:
        a.setflags(write=False)
    return out


def restatement_inputs(th, sl, locs, X, lp, Xp):
    """(Cq, dq, d) by the rule's wording, from the public covariance entry alone"""
    import cocons_amd as ca
    Cq = np.asarray(ca.cov_rns_pred(th, locs, lp, X, Xp, sl))
    dq = np.diagonal(np.asarray(ca.cov_rns_pred(th, lp, lp, Xp, Xp, sl))).copy()
    d = np.diagonal(np.asarray(ca.cov_rns_pred(th, locs, locs, X, X, sl))).copy()
    return Cq, dq, d


def check_all_shapes(f, th, sl, locs, X, lp, Xp, shapes=SHAPES):
    import cocons_amd as ca
    Cq, dq, d = restatement_inputs(th, sl, locs, X, lp, Xp)
    mp, tables = lp.shape[0], 0
    for mc, hops in shapes:
        first = ca.vecchia_neighbours_pred_device(locs, lp, mc)
        lists = ca.vecchia_neighbours_pred_device(locs, locs, mc)
        ms = _ms(mc, hops)
        want = ca.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, ms[-1], hops)
        for m in ms:
            got = f.neighbours_corr_pred(th, lp, Xp, m, m_cand=mc, hops=hops)
            assert got.shape == (mp, m) and got.dtype == np.int32
            bad = np.flatnonzero(np.any(got != want[:, :m], axis=1))
            assert bad.size == 0, ("n %d mp %d m_cand %d hops %d m %d: %d rows differ, first row %d: %s vs %s"
                                   % (locs.shape[0], mp, mc, hops, m, bad.size, bad[0] + 1, got[bad[0]], want[bad[0], :m]))
            tables += 1
    return tables


def _design(locs):
    from cocons_amd import workloads as wl
    return np.asfortranarray(wl.design_from_locs(locs)["std.covs"])


@pytest.mark.parametrize("n,mp", SIZES)
@pytest.mark.parametrize("which", ["bessel", "closed", "fixed"])
def test_table_is_the_restatement_integer_for_integer(data, which, n, mp):
    import cocons_amd as ca
    th, sl = _thetas()[which]
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    lp, Xp = data[3][:mp], np.asfortranarray(data[4][:mp])
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        tables = check_all_shapes(f, th, sl, locs, X, lp, Xp)
        print("corr-pred-report gpu | %s theta, n %d, mp %d | %d tables over m_cand x hops x m against the restatement | "
              "rows that differ 0" % (which, n, mp, tables))
        if n <= 30:
            # n <= m_cand: every observation is ranked
            got = f.neighbours_corr_pred(th, lp, Xp, 30, m_cand=30, hops=1)
            assert all(set(r[r > 0]) == set(range(1, n + 1)) for r in got)
    finally:
        f.close()


def test_lattice_ties_coincident_sites_on_observations_and_far_outside(data):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    th, sl = _thetas()["bessel"]
    rng = np.random.default_rng(11)
    iso = CR.theta_iso()
    iso["nugget"] = np.array([np.log(0.05)])
    lat = CR.lattice_ties()[0] / 11.0
    # new sites at the centres of lattice cells (four observations at exactly the same distance) and on lattice points
    centres = (np.column_stack([rng.integers(0, 11, 40), rng.integers(0, 11, 40)]) + 0.5) / 11.0
    cases = {"lattice": (lat, np.ones((144, 1), order="F"), iso, wl.SMOOTH_LIMITS, np.vstack([centres, lat[:25]]),
                         np.ones((65, 1), order="F"))}
    co = CR.coincident()[0]
    Xco = _design(co)
    pick = rng.permutation(90)[:40]
    # on top of observations (with their covariates: rho of the twin is that of the site with itself), and coincident ones
    cases["coincident"] = (co, Xco, th, sl, co[pick].copy(), np.asfortranarray(Xco[pick]))
    locs, X = data[0][:300], np.asfortranarray(data[1][:300])
    on = np.vstack([locs[:30], data[3][:10]])
    cases["on observations"] = (locs, X, th, sl, on, np.asfortranarray(np.vstack([X[:30], data[4][:10]])))
    far = np.array([[5.0, 5.0], [-3.0, 0.5], [0.5, 40.0], [-20.0, -20.0], [1.0 + 1e-9, 0.5], [1e6, 0.0]])
    # (with covariates of sites inside: the link functions of the far coordinates themselves overflow.  At the last site every
    # correlation underflows to 0: the key falls back on the index)
    cases["far outside"] = (locs, X, th, sl, far, np.asfortranarray(data[4][:6]))
    for name, (locs_, X_, t, lim, lp, Xp) in cases.items():
        n = locs_.shape[0]
        f = ca.CoconsVecchiaFit.from_knn(locs_, X_, np.zeros(n), lim, 5)
        try:
            tables = check_all_shapes(f, t, lim, locs_, X_, lp, Xp, shapes=[(5, 1), (5, 2), (30, 2), (63, 2)])
            print("corr-pred-report gpu | %s, n %d, mp %d | %d tables against the restatement | rows that differ 0"
                  % (name, n, lp.shape[0], tables))
            if name == "on observations":
                got = f.neighbours_corr_pred(t, lp, Xp, 5, m_cand=5, hops=2)
                assert np.array_equal(got[:30, 0], np.arange(1, 31))          # the observation under the site comes first
            if name == "lattice":
                got = f.neighbours_corr_pred(t, lp, Xp, 12, m_cand=12, hops=2)
                Cq, dq, d = restatement_inputs(t, lim, locs_, X_, lp, Xp)
                ties = 0
                for q in range(lp.shape[0]):
                    row = got[q][got[q] > 0] - 1
                    rho = Cq[q, row] / np.sqrt(dq[q] * d[row])
                    same = np.diff(rho) == 0
                    assert np.all(np.diff(rho) <= 0) and np.all(np.diff(row)[same] > 0)
                    ties += int(same.sum())
                assert ties > 20, ties
                print("corr-pred-report gpu | lattice | exact ties of rho inside the rows of one table, all to the lower index: %d"
                      % ties)
        finally:
            f.close()


def test_repeated_calls_other_widths_in_between_prefixes_and_what_the_handle_keeps(data):
    import cocons_amd as ca
    th, sl = _thetas()["bessel"]
    n = 300
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    lp, Xp = data[3][:65], np.asfortranarray(data[4][:65])
    th0 = dict(th, mean=np.zeros(3))
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 10)
    try:
        val0, parts0 = f.neg2loglik_core(th0)
        pk0 = f.predict_knn_core(th0, lp, Xp, 10)          # (builds the grid: the bytes below count it already)
        b0 = f.info()["bytes"]
        one = f.neighbours_corr_pred(th, lp, Xp, 30, m_cand=30, hops=1)
        assert f.info()["bytes"] == b0                       # one hop keeps nothing
        a = f.neighbours_corr_pred(th, lp, Xp, 30, m_cand=30, hops=2)
        assert f.info()["bytes"] == b0 + 4 * n * 30          # the all-observations table, once
        for _ in range(3):
            assert np.array_equal(f.neighbours_corr_pred(th, lp, Xp, 30, m_cand=30, hops=2), a)
        assert f.info()["bytes"] == b0 + 4 * n * 30
        c = f.neighbours_corr_pred(th, lp, Xp, 7, m_cand=12, hops=2)
        assert f.info()["bytes"] == b0 + 4 * n * 12          # made again at the other width
        assert np.array_equal(f.neighbours_corr_pred(th, lp, Xp, 30, m_cand=30, hops=2), a)
        assert np.array_equal(f.neighbours_corr_pred(th, lp, Xp, 7, m_cand=12, hops=2), c)
        assert np.array_equal(f.neighbours_corr_pred(th, lp, Xp, 30, m_cand=30, hops=1), one)
        # prefixes; the default m_cand = min(2 m, 63), two hops
        assert np.array_equal(f.neighbours_corr_pred(th, lp, Xp, 7, m_cand=30, hops=2), a[:, :7])
        assert np.array_equal(f.neighbours_corr_pred(th, lp, Xp, 15), a[:, :15])
        # one hop with m = m_cand: the Euclidean set
        P = ca.vecchia_neighbours_pred_device(locs, lp, 30)
        assert np.array_equal(np.sort(one, axis=1), np.sort(P, axis=1))
        # a row depends on no other row of the query set
        sub = f.neighbours_corr_pred(th, lp[40:43], np.asfortranarray(Xp[40:43]), 30, m_cand=30, hops=2)
        assert np.array_equal(sub, a[40:43])
        # and the handle's other entries keep their bits
        val1, parts1 = f.neg2loglik_core(th0)
        assert val1 == val0 and np.array_equal(parts1, parts0)
        pk1 = f.predict_knn_core(th0, lp, Xp, 10)
        assert all(np.array_equal(u, v) for u, v in zip(pk0, pk1))
    finally:
        f.close()


def test_isotropic_theta_returns_the_euclidean_sets(data):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 300
    locs, lp = data[0][:n], data[3][:65]
    X, Xp = np.ones((n, 1), order="F"), np.ones((65, 1), order="F")
    iso = CR.theta_iso()
    iso["nugget"] = np.array([np.log(0.05)])
    f = ca.CoconsVecchiaFit.from_knn(locs, X, np.zeros(n), wl.SMOOTH_LIMITS, 5)
    try:
        P = ca.vecchia_neighbours_pred_device(locs, lp, 10)
        for mc, hops in ((10, 1), (10, 2), (30, 2), (20, 1)):
            got = f.neighbours_corr_pred(iso, lp, Xp, 10, m_cand=mc, hops=hops)
            # (random sites: no two distances tie, and rho is strictly monotone in them well above its rounding)
            assert np.array_equal(np.sort(got, axis=1), np.sort(P, axis=1)), (mc, hops)
    finally:
        f.close()


def test_refusals_that_need_a_live_handle_and_a_rho_that_is_not_finite(data):
    import cocons_amd as ca
    from cocons_amd import _lib, host
    L = _lib.load()
    th, sl = _thetas()["bessel"]
    n, mp = 64, 9
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    lp, Xp = np.asfortranarray(data[3][:mp]), np.asfortranarray(data[4][:mp])
    name = "cocons_vecchia_neighbours_corr_pred"
    nn = np.full((mp, 4), -7, dtype=np.int32, order="F")
    st, qf = np.full(mp, -7.0), np.full(mp, -7.0)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)      # noqa: E731

    def call(h, T):
        return L.cocons_vecchia_neighbours_corr_pred(h, dp(T), mp, dp(lp), dp(Xp), 5, 2, 4, nn.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def predict(h, T):
        return L.cocons_vecchia_predict_corr_knn(h, dp(T), dp(np.zeros(3)), 0, mp, dp(lp), dp(Xp), 5, 2, 4, dp(st), dp(qf))

    T = host.theta_table(th)
    dense = ca.CoconsFit(locs, X, z, sl)
    try:
        assert call(dense._h, T) == -1 and _lib.last_error().startswith(name + ": not a Vecchia fit")
        assert predict(dense._h, T) == -1 and _lib.last_error().startswith("cocons_vecchia_predict_corr_knn: not a Vecchia fit")
    finally:
        dense.close()
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        for k, v in ((0, np.nan), (7, np.inf), (17, -np.inf)):
            Tb = T.copy()
            Tb.ravel()[k] = v
            assert call(f._h, Tb) == -1 and _lib.last_error().startswith("%s: theta[%d] is not finite" % (name, k))
            assert predict(f._h, Tb) == -1
            assert _lib.last_error().startswith("cocons_vecchia_predict_corr_knn: theta[%d] is not finite" % k)
        assert L.cocons_vecchia_predict_corr_knn(f._h, dp(T), dp(np.zeros(3)), 1, mp, dp(lp), dp(Xp), 5, 2, 4, dp(st), dp(qf)) == -1
        assert "z_col" in _lib.last_error()
        # a finite theta whose variances overflow: every rho is NaN or infinite, row 1 is the first with a candidate
        big = {k: np.array(v, dtype=float) for k, v in th.items()}
        big["std.dev"][0] = 1500.0
        assert call(f._h, host.theta_table(big)) == 1
        assert _lib.last_error().startswith(name + ": row 1 ")
        assert predict(f._h, host.theta_table(big)) == 1
        assert _lib.last_error().startswith("cocons_vecchia_predict_corr_knn: row 1 ")
        assert np.all(nn == -7) and np.all(st == -7.0) and np.all(qf == -7.0)
        with pytest.raises(_lib.CholeskyError):
            f.neighbours_corr_pred(big, lp, Xp, 4, m_cand=5, hops=2)
        # and the handle serves on
        assert call(f._h, T) == 0 and np.all(nn > 0)
        assert predict(f._h, T) == 0 and np.all(np.isfinite(st)) and np.all(qf > 0)
    finally:
        f.close()
