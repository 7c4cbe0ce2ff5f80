"""The numpy restatement of the rule of the Vecchia neighbours by model correlation (host.vecchia_neighbours_corr)
against the brute-force statement of corr_knn_reference.py, and what the rule buys: the KL condition on the oracle's covariance.
No GPU."""
import numpy as np
import pytest

import corr_knn_reference as CR
import knn_reference as KR
from cocons_amd import host


def _rows_as_sets(nn):
    return [frozenset(int(v) for v in row if v > 0) for row in np.asarray(nn)]


@pytest.fixture(scope="module")
def random_case():
    locs = np.random.default_rng(11).uniform(0, 1, size=(160, 2))
    return locs, CR.aniso_exp(locs)


@pytest.mark.parametrize("m_cand,hops,m", [(1, 1, 1), (1, 2, 1), (1, 2, 2), (5, 1, 5), (5, 2, 5), (5, 2, 30), (12, 2, 12),
                                           (30, 1, 7), (30, 2, 63), (63, 2, 63)])
def test_restatement_is_the_brute_force_on_random_sites(random_case, m_cand, hops, m):
    locs, S = random_case
    cand = KR.brute_self(locs, m_cand)
    got = host.vecchia_neighbours_corr(S, cand, m, hops)
    assert got.dtype == np.int32 and got.shape == (locs.shape[0], m)
    assert np.array_equal(got, CR.brute(S, cand, m, hops))
    # a row ranks all its predecessors while the Euclidean table still holds them all
    for i in range(min(m_cand + 1, locs.shape[0])):
        assert (got[i] > 0).sum() == min(i, m) and np.all(got[i] <= i)
    # rows with fewer than m unique candidates are zero-padded behind them
    nz = (got > 0).sum(axis=1)
    assert all(np.all(got[i, :nz[i]] > 0) and np.all(got[i, nz[i]:] == 0) for i in range(got.shape[0]))
    if m > m_cand + m_cand * m_cand * (hops - 1):
        assert nz.max() < m


def test_ties_go_to_the_lower_index_on_a_lattice():
    locs, S = CR.lattice_ties()
    for m_cand, hops, m in ((8, 1, 4), (8, 2, 6), (20, 2, 9)):
        cand = KR.brute_self(locs, m_cand)
        got = host.vecchia_neighbours_corr(S, cand, m, hops)
        assert np.array_equal(got, CR.brute(S, cand, m, hops))
        ties = 0
        for i in range(got.shape[0]):
            row = got[i][got[i] > 0] - 1
            rho = S[row, i] / np.sqrt(S[i, i] * S[row, row])
            assert np.all(np.diff(rho) <= 0)
            same = np.diff(rho) == 0
            assert np.all(np.diff(row)[same] > 0)
            ties += int(same.sum())
        assert ties > 50                           # (the case does what it is there for)


def test_coincident_sites():
    locs, S = CR.coincident()
    for m_cand, hops, m in ((4, 1, 4), (4, 2, 10), (15, 2, 15)):
        cand = KR.brute_self(locs, m_cand)
        assert np.array_equal(host.vecchia_neighbours_corr(S, cand, m, hops), CR.brute(S, cand, m, hops))


def test_prefix_property_and_one_hop_is_the_euclidean_set(random_case):
    locs, S = random_case
    for m_cand, hops in ((9, 1), (9, 2), (30, 2)):
        cand = KR.brute_self(locs, m_cand)
        wide = host.vecchia_neighbours_corr(S, cand, 40 if hops == 2 else m_cand, hops)
        for m in (1, 3, m_cand):
            assert np.array_equal(host.vecchia_neighbours_corr(S, cand, m, hops), wide[:, :m])
    cand = KR.brute_self(locs, 9)
    assert _rows_as_sets(host.vecchia_neighbours_corr(S, cand, 9, 1)) == _rows_as_sets(cand)


def test_a_correlation_that_is_not_finite_names_its_row(random_case):
    locs, S = random_case
    S = S.copy()
    S[40, 40] = np.inf
    S[17, 17] = np.nan
    with pytest.raises(ValueError, match="row 18 "):
        host.vecchia_neighbours_corr(S, KR.brute_self(locs, 5), 3, 2)
    with pytest.raises(ValueError):
        host.vecchia_neighbours_corr(S, KR.brute_self(locs, 5), 3, 3)


# ---- the KL condition: n = 400, m = 10, random order, the oracle's covariance ----------------------------------------------
N_KL, M_KL = 400, 10


@pytest.fixture(scope="module")
def kl_sites():
    from oracle import oracle as O
    O.build()
    locs = np.random.default_rng(20260400).uniform(0, 1, size=(N_KL, 2))
    return O, locs, KR.brute_self(locs, M_KL)


def test_kl_anisotropic_every_setting_is_strictly_below_the_euclidean_table(kl_sites):
    O, locs, euclid = kl_sites
    S = O.cov_rns(CR.theta_aniso(), locs, np.ones((N_KL, 1), order="F"), (0.5, 2.5))
    half_logdet = float(np.sum(np.log(np.diag(np.linalg.cholesky(S)))))
    base = CR.kl(S, euclid, half_logdet)
    print("KL, Euclidean table: %.4f" % base)
    for m_cand, hops in CR.SETTINGS:
        mc = CR.scaled(m_cand, M_KL)
        got = CR.kl(S, host.vecchia_neighbours_corr(S, KR.brute_self(locs, mc), M_KL, hops), half_logdet)
        print("KL, m_cand = %d, hops = %d: %.4f (%.3f of the Euclidean table's)" % (mc, hops, got, got / base))
        assert got < base, (mc, hops, got, base)


def test_kl_isotropic_the_tables_are_the_euclidean_table_as_sets(kl_sites):
    O, locs, euclid = kl_sites
    S = O.cov_rns(CR.theta_iso(), locs, np.ones((N_KL, 1), order="F"), (0.5, 2.5))
    want = _rows_as_sets(euclid)
    for m_cand, hops in CR.SETTINGS:
        mc = CR.scaled(m_cand, M_KL)
        assert _rows_as_sets(host.vecchia_neighbours_corr(S, KR.brute_self(locs, mc), M_KL, hops)) == want, (mc, hops)
