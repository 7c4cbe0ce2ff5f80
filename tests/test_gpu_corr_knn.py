"""cocons_vecchia_neighbours_corr on the device against the numpy restatement of its rule
(host.vecchia_neighbours_corr), integer for integer: the restatement is fed the device's own cocons_cov_rns matrix for that theta
and the Euclidean table of cocons_vecchia_neighbours.  Sizes around the wavefront (1, 2, 64, 65) and several hundred rows, every
width of the candidate table at which the set in LDS changes its size, one and two hops, m = 1, m_cand and 63, a theta on the
Bessel branch and one at a closed-form smoothness, each with covariate-driven anisotropy; a lattice with exact ties, coincident
sites and an order sorted by x (two-hop sets that barely grow); repeated calls; the handle untouched; the refusals that need a
live handle; and, so that the device is not only compared with itself, the selection pinned to the CPU oracle's correlations."""
import ctypes

import numpy as np
import pytest

import corr_knn_reference as CR
import knn_reference as KR

pytestmark = pytest.mark.gpu

N = 700
SHAPES = [(mc, hops) for mc in (1, 5, 30, 63) for hops in (1, 2)]


def _ms(mc, hops):
    cap = min(4032, mc + mc * mc * (hops - 1))
    return sorted(m for m in {1, mc, 63} if m <= cap)


def _thetas():
    from cocons_amd import workloads as wl
    closed = CR.theta_covariate()
    closed["smooth"] = np.zeros(3)
    return {"bessel": (CR.theta_covariate(), wl.SMOOTH_LIMITS), "closed": (closed, (1.5, 1.5))}


@pytest.fixture(scope="module")
def data():
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(20260321)
    locs = rng.uniform(0, 1, size=(N, 2))
    X = np.asfortranarray(wl.design_from_locs(locs)["std.covs"])
    return locs, X, rng.standard_normal(N)


_S = {}


def _cov(key, th, locs, X, sl):
    """the device's covariance of a case, computed once"""
    import cocons_amd as ca
    if key not in _S:
        _S[key] = np.asarray(ca.cov_rns(th, locs, X, sl))
        _S[key].setflags(write=False)
    return _S[key]


def _check_all_shapes(f, th, S, locs, shapes=SHAPES):
    import cocons_amd as ca
    n, tables = locs.shape[0], 0
    for mc, hops in shapes:
        cand = ca.vecchia_neighbours_device(locs, mc)
        ms = _ms(mc, hops)
        want = ca.vecchia_neighbours_corr(S, cand, ms[-1], hops)
        for m in ms:
            got = f.neighbours_corr(th, m, m_cand=mc, hops=hops)
            assert got.shape == (n, m) and got.dtype == np.int32
            bad = np.flatnonzero(np.any(got != want[:, :m], axis=1))
            assert bad.size == 0, ("n %d m_cand %d hops %d m %d: %d rows differ, first row %d: %s vs %s"
                                   % (n, mc, hops, m, bad.size, bad[0] + 1, got[bad[0]], want[bad[0], :m]))
            tables += 1
    return tables


@pytest.mark.parametrize("n", [1, 2, 64, 65, 300, 700])
@pytest.mark.parametrize("which", ["bessel", "closed"])
def test_table_is_the_restatement_integer_for_integer(data, which, n):
    import cocons_amd as ca
    th, sl = _thetas()[which]
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    S = _cov((which, n), th, locs, X, sl).reshape(n, n)
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        tables = _check_all_shapes(f, th, S, locs)
        print("corr-report gpu | %s theta, n %d | %d tables over m_cand x hops x m against the restatement | rows that differ 0"
              % (which, n, tables))
    finally:
        f.close()


def test_sorted_by_x_lattice_ties_and_coincident_sites(data):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    th, sl = _thetas()["bessel"]
    # sorted by x: the predecessors all lie to one side, the lists of a row's neighbours nearly coincide
    o = np.argsort(data[0][:300, 0], kind="stable")
    cases = {"sorted": (data[0][:300][o], np.asfortranarray(data[1][:300][o]), th, sl)}
    # a lattice under a stationary isotropic theta: rho ties exactly along the axes; and every site three times over
    iso = CR.theta_iso()
    iso["nugget"] = np.array([np.log(0.05)])
    lat = CR.lattice_ties()[0] / 11.0
    cases["lattice"] = (lat, np.ones((lat.shape[0], 1), order="F"), iso, wl.SMOOTH_LIMITS)
    co = CR.coincident()[0]
    cases["coincident"] = (co, np.asfortranarray(wl.design_from_locs(co)["std.covs"]), th, sl)
    for name, (locs, X, t, lim) in cases.items():
        n = locs.shape[0]
        S = _cov(name, t, locs, X, lim).reshape(n, n)
        f = ca.CoconsVecchiaFit.from_knn(locs, X, np.zeros(n), lim, 5)
        try:
            tables = _check_all_shapes(f, t, S, locs, shapes=[(5, 1), (5, 2), (30, 2), (63, 2)])
            print("corr-report gpu | %s, n %d | %d tables against the restatement | rows that differ 0" % (name, n, tables))
            if name == "lattice":
                got = f.neighbours_corr(t, 12, m_cand=12, hops=2)
                ties = 0
                for i in range(n):
                    row = got[i][got[i] > 0] - 1
                    rho = S[row, i] / np.sqrt(S[i, i] * S[row, row])
                    same = np.diff(rho) == 0
                    assert np.all(np.diff(rho) <= 0) and np.all(np.diff(row)[same] > 0)
                    ties += int(same.sum())
                assert ties > 20, ties
                print("corr-report gpu | lattice | exact ties of rho inside the rows of one table, all to the lower index: %d" % ties)
        finally:
            f.close()


def test_repeated_calls_prefixes_and_the_handle_untouched(data):
    import cocons_amd as ca
    th, sl = _thetas()["bessel"]
    n = 300
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    th0 = dict(th, mean=np.zeros(3))
    B = np.asfortranarray(np.random.default_rng(4).standard_normal((n, 2)))
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 10)
    try:
        val0, parts0 = f.neg2loglik_core(th0)
        w0 = f.whiten_core(th0, B)
        info0 = f.info()
        a = f.neighbours_corr(th, 30, m_cand=30, hops=2)
        for _ in range(3):
            assert np.array_equal(f.neighbours_corr(th, 30, m_cand=30, hops=2), a)
        assert np.array_equal(f.neighbours_corr(th, 7, m_cand=30, hops=2), a[:, :7])
        # defaults: m_cand = min(2 m, 63), two hops
        assert np.array_equal(f.neighbours_corr(th, 15), a[:, :15])
        # rows that still see all their predecessors rank them all
        assert all(set(a[i][a[i] > 0]) == set(range(1, i + 1)) for i in range(31))
        assert f.info() == info0
        val1, parts1 = f.neg2loglik_core(th0)
        assert val1 == val0 and np.array_equal(parts1, parts0)
        w1 = f.whiten_core(th0, B)
        assert all(np.array_equal(u, v) for u, v in zip(w0, w1))
    finally:
        f.close()


def test_selection_against_the_cpu_oracle_correlations(data):
    """In every row the smallest selected rho is >= the largest non-selected candidate's rho - 1e-12 under the ORACLE's
    correlations: a tolerance on rho in [0, 1] well above the pair arithmetic's documented agreement with the oracle
    (2e-12 entrywise on entries of size sigma^2, relative to a diagonal above it).  No row is excused."""
    import cocons_amd as ca
    from oracle import oracle as O
    O.build()
    n = 300
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    for which, (th, sl) in _thetas().items():
        S = O.cov_rns(th, locs, X, sl)
        d = np.sqrt(np.diag(S))
        Rho = S / np.outer(d, d)
        f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
        try:
            for mc, hops, m in ((30, 2, 30), (60, 1, 30), (12, 2, 12)):
                got = f.neighbours_corr(th, m, m_cand=mc, hops=hops)
                cand = KR.brute_self(locs, mc)
                worst = 0.0
                for i in range(n):
                    c = cand[i][cand[i] > 0]
                    if hops == 2 and c.size:
                        c = np.concatenate([c, cand[c - 1].ravel()])
                    C = set(int(v) for v in c if v > 0)
                    sel = set(int(v) for v in got[i] if v > 0)
                    assert sel <= C and len(sel) == min(m, len(C)), (which, mc, hops, i)
                    rest = C - sel
                    if sel and rest:
                        gap = max(Rho[j - 1, i] for j in rest) - min(Rho[j - 1, i] for j in sel)
                        worst = max(worst, gap)
                        assert gap <= 1e-12, (which, mc, hops, i + 1, gap)
                print("corr-report oracle pin | %s m_cand%d hops%d m%d | worst (largest left out - smallest taken) %.2e"
                      % (which, mc, hops, m, worst))
        finally:
            f.close()


def test_refusals_that_need_a_live_handle_and_a_rho_that_is_not_finite(data):
    import cocons_amd as ca
    from cocons_amd import _lib, host
    L = _lib.load()
    th, sl = _thetas()["bessel"]
    n = 64
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    name = "cocons_vecchia_neighbours_corr"
    nn = np.full((n, 4), -7, dtype=np.int32, order="F")

    def call(h, T):
        return L.cocons_vecchia_neighbours_corr(h, T.ctypes.data_as(_lib.c_dp), 5, 2, 4, nn.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    T = host.theta_table(th)
    dense = ca.CoconsFit(locs, X, z, sl)
    try:
        assert call(dense._h, T) == -1 and _lib.last_error().startswith(name + ": not a Vecchia fit")
    finally:
        dense.close()
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        for k, v in ((0, np.nan), (7, np.inf), (17, -np.inf)):
            Tb = T.copy()
            Tb.ravel()[k] = v
            assert call(f._h, Tb) == -1 and _lib.last_error().startswith("%s: theta[%d] is not finite" % (name, k))
        # a finite theta whose variances overflow: every rho is NaN or infinite, row 2 is the first with a candidate
        big = {k: np.array(v, dtype=float) for k, v in th.items()}
        big["std.dev"][0] = 1500.0
        assert call(f._h, host.theta_table(big)) == 2
        assert _lib.last_error().startswith(name + ": row 2 ")
        assert np.all(nn == -7)
        with pytest.raises(_lib.CholeskyError):
            f.neighbours_corr(big, 4, m_cand=5, hops=2)
        with pytest.raises(_lib.CoconsHipError, match="cocons_fit_create_vecchia_corr_knn: row 2 "):
            ca.CoconsVecchiaFit.from_corr_knn(locs, X, z, sl, big, 4, m_cand=5, hops=2)
        # and the handle serves on
        assert call(f._h, T) == 0 and np.all(nn[1:, 0] > 0) and np.all(nn[0] == 0)
    finally:
        f.close()
