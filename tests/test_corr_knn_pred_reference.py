"""The numpy restatement of the rule of the neighbours of new locations by model correlation
(host.vecchia_neighbours_corr_pred) against the brute-force statement of corr_knn_pred_reference.py, the
properties the header states, and what the rule buys: the variance condition on the oracle's covariance.  No GPU."""
import numpy as np
import pytest

import corr_knn_pred_reference as PR
import corr_knn_reference as CR
import knn_reference as KR
from cocons_amd import host


def _rows_as_sets(nn):
    return [frozenset(int(v) for v in row if v > 0) for row in np.asarray(nn)]


@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(12)
    locs = rng.uniform(0, 1, size=(160, 2))
    q = np.vstack([rng.uniform(-0.1, 1.1, size=(50, 2)), locs[[3, 77, 159]]])          # the last three ON observations
    return locs, q, PR.aniso_cross(locs, q)


@pytest.mark.parametrize("m_cand,hops,m", [(1, 1, 1), (1, 2, 1), (1, 2, 2), (5, 1, 5), (5, 2, 5), (5, 2, 30), (12, 2, 12),
                                           (30, 1, 7), (30, 2, 63), (63, 2, 63)])
def test_restatement_is_the_brute_force_on_random_sites(random_case, m_cand, hops, m):
    locs, q, (Cq, dq, d) = random_case
    first, lists = KR.brute_pred(locs, q, m_cand), KR.brute_pred(locs, locs, m_cand)
    got = host.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, m, hops)
    assert got.dtype == np.int32 and got.shape == (q.shape[0], m) and got.flags.f_contiguous
    assert np.array_equal(got, PR.brute(Cq, dq, d, first, lists, m, hops))
    # rows with fewer than m unique candidates are zero-padded behind them
    nz = (got > 0).sum(axis=1)
    assert all(np.all(got[i, :nz[i]] > 0) and np.all(got[i, nz[i]:] == 0) for i in range(got.shape[0]))
    assert nz.min() >= min(m, m_cand)
    if m > m_cand + m_cand * m_cand * (hops - 1):
        assert nz.max() < m
    # a new site on an observation ranks that observation first: its rho is 1, every other below 1 / (1 + nugget)
    assert list(got[-3:, 0]) == [4, 78, 160]
    # one hop never reads the second table
    if hops == 1:
        assert np.array_equal(host.vecchia_neighbours_corr_pred(Cq, dq, d, first, None, m, 1), got)


def test_ties_go_to_the_lower_index_on_a_lattice():
    locs, _ = CR.lattice_ties()
    rng = np.random.default_rng(5)
    q = np.vstack([np.column_stack([rng.integers(0, 11, 30), rng.integers(0, 11, 30)]) + 0.5, locs[:10]])
    Cq, dq, d = PR.lattice_cross(locs, q)
    for m_cand, hops, m in ((8, 1, 4), (8, 2, 6), (20, 2, 9)):
        first, lists = KR.brute_pred(locs, q, m_cand), KR.brute_pred(locs, locs, m_cand)
        got = host.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, m, hops)
        assert np.array_equal(got, PR.brute(Cq, dq, d, first, lists, m, hops))
        ties = 0
        for i in range(got.shape[0]):
            row = got[i][got[i] > 0] - 1
            rho = Cq[i, row] / np.sqrt(dq[i] * d[row])
            assert np.all(np.diff(rho) <= 0)
            same = np.diff(rho) == 0
            assert np.all(np.diff(row)[same] > 0)
            ties += int(same.sum())
        assert ties > 50                           # (the case does what it is there for)
        assert np.array_equal(got[30:, 0], np.arange(1, 11))


def test_coincident_observations_and_new_sites_on_them():
    locs, _ = CR.coincident()
    rng = np.random.default_rng(6)
    q = np.vstack([rng.uniform(0, 1, size=(20, 2)), locs[:15]])
    Cq, dq, d = PR.aniso_cross(locs, q, nugget=0.05)
    for m_cand, hops, m in ((4, 1, 4), (4, 2, 10), (15, 2, 15)):
        first, lists = KR.brute_pred(locs, q, m_cand), KR.brute_pred(locs, locs, m_cand)
        got = host.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, m, hops)
        assert np.array_equal(got, PR.brute(Cq, dq, d, first, lists, m, hops))
        # the three observations under the site come first, lowest index first (m_cand >= 3 holds all three)
        for i in range(15):
            twins = np.flatnonzero(np.all(locs == locs[i], axis=1)) + 1
            assert np.array_equal(got[20 + i, :3], twins[:3])


def test_prefix_property_one_hop_is_the_euclidean_set_and_few_observations(random_case):
    locs, q, (Cq, dq, d) = random_case
    for m_cand, hops in ((9, 1), (9, 2), (30, 2)):
        first, lists = KR.brute_pred(locs, q, m_cand), KR.brute_pred(locs, locs, m_cand)
        wide = host.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, 40 if hops == 2 else m_cand, hops)
        for m in (1, 3, m_cand):
            assert np.array_equal(host.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, m, hops), wide[:, :m])
    first = KR.brute_pred(locs, q, 9)
    assert _rows_as_sets(host.vecchia_neighbours_corr_pred(Cq, dq, d, first, None, 9, 1)) == _rows_as_sets(first)
    # n <= m_cand: every observation is ranked, with one hop and with two
    few = locs[:7]
    Cf, dqf, df = PR.aniso_cross(few, q)
    first, lists = KR.brute_pred(few, q, 12), KR.brute_pred(few, few, 12)
    for hops in (1, 2):
        got = host.vecchia_neighbours_corr_pred(Cf, dqf, df, first, lists, 12, hops)
        assert _rows_as_sets(got) == [frozenset(range(1, 8))] * q.shape[0] and np.all(got[:, 7:] == 0)


def test_isotropic_covariance_returns_the_euclidean_sets(random_case):
    locs, q, _ = random_case
    Cq, dq, d = PR.aniso_cross(locs, q, ratio=1.0)
    want = _rows_as_sets(KR.brute_pred(locs, q, 10))
    for m_cand, hops in ((10, 1), (20, 1), (10, 2), (30, 2)):
        first, lists = KR.brute_pred(locs, q, m_cand), KR.brute_pred(locs, locs, m_cand)
        assert _rows_as_sets(host.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, 10, hops)) == want, (m_cand, hops)


def test_a_correlation_that_is_not_finite_names_its_row(random_case):
    locs, q, (Cq, dq, d) = random_case
    first, lists = KR.brute_pred(locs, q, 5), KR.brute_pred(locs, locs, 5)
    bad = dq.copy()
    bad[17] = np.nan
    bad[40] = np.inf
    with pytest.raises(ValueError, match="row 18 "):
        host.vecchia_neighbours_corr_pred(Cq, bad, d, first, lists, 3, 2)
    with pytest.raises(ValueError):
        host.vecchia_neighbours_corr_pred(Cq, dq, d, first, lists, 3, 3)


# ---- the variance condition: n = 900, 150 new sites, m = 30, the oracle's covariance -----------------------------------------
N_VAR, MP_VAR, M_VAR = 900, 150, 30


@pytest.fixture(scope="module")
def var_sites():
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(20260500)
    return O, rng.uniform(0, 1, size=(N_VAR, 2)), rng.uniform(0, 1, size=(MP_VAR, 2))


def _oracle_case(O, th, locs, q):
    """(S, Cp, the new sites' variances, the rule's diagonals) from the oracle, intercept only"""
    sl = (0.5, 2.5)
    X, Xp = np.ones((locs.shape[0], 1), order="F"), np.ones((q.shape[0], 1), order="F")
    S = O.cov_rns(th, locs, X, sl)
    Cp = O.cov_rns_pred(th, locs, q, X, Xp, sl)
    dq = np.diagonal(O.cov_rns_pred(th, q, q, Xp, Xp, sl)).copy()
    d = np.diagonal(O.cov_rns_pred(th, locs, locs, X, X, sl)).copy()
    var = 1 / np.exp(-(Xp @ th["std.dev"])) + np.exp(Xp @ th["nugget"])          # cocoPredict's (R/predict.R:170-171)
    return S, Cp, var, dq, d


def test_variance_anisotropic_the_30_2_table_is_strictly_below_the_euclidean_table(var_sites):
    """Measured (tests/golden/VECCHIA_CORR_PRED_REPORT.md): the mean excess of the local-kriging variance over the exact one
    is 2.55 % for the Euclidean table and 0.27 % for the (30, 2) table (worst site: 32.7 % and 2.9 %)."""
    O, locs, q = var_sites
    S, Cp, var, dq, d = _oracle_case(O, CR.theta_aniso(5.0), locs, q)
    base = PR.excess_variance(S, Cp, var, KR.brute_pred(locs, q, M_VAR))
    print("excess variance, Euclidean table: mean %.4e worst %.4e" % base)
    nn = host.vecchia_neighbours_corr_pred(Cp, dq, d, KR.brute_pred(locs, q, 30), KR.brute_pred(locs, locs, 30), M_VAR, 2)
    got = PR.excess_variance(S, Cp, var, nn)
    print("excess variance, m_cand = 30, hops = 2: mean %.4e worst %.4e" % got)
    assert got[0] < base[0], (got, base)


def test_variance_isotropic_the_tables_are_equal_as_sets_and_no_worse(var_sites):
    O, locs, q = var_sites
    S, Cp, var, dq, d = _oracle_case(O, CR.theta_iso(), locs, q)
    euclid = KR.brute_pred(locs, q, M_VAR)
    base = PR.excess_variance(S, Cp, var, np.sort(euclid, axis=1))          # (both ascending: the same sums in the same order)
    nn = host.vecchia_neighbours_corr_pred(Cp, dq, d, KR.brute_pred(locs, q, 30), KR.brute_pred(locs, locs, 30), M_VAR, 2)
    assert _rows_as_sets(nn) == _rows_as_sets(euclid)
    got = PR.excess_variance(S, Cp, var, np.sort(nn, axis=1))
    print("excess variance, isotropic: Euclidean mean %.4e, (30, 2) mean %.4e" % (base[0], got[0]))
    assert got[0] <= base[0], (got, base)
