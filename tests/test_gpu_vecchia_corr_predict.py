"""cocons_vecchia_predict_corr_knn on the device: local kriging on the neighbours of the new locations by model
correlation.  To the bit cocons_vecchia_predict fed with the table of cocons_vecchia_neighbours_corr_pred, at sizes around the
wavefront and several hundred rows; over more rows than a chunk holds a row's outputs depend neither on the chunking nor on
the other rows; the existing prediction entries on the same handle keep their bits; and, so that the device is not only
compared with itself, the prediction is pinned to a numpy local kriging on the CPU oracle's matrices.

Bound of the comparison with the oracle: the project's parity bound PARITY = 1e-8 (test_gpu_dense_sizes), relative to the
largest magnitude of the compared array -- the bound test_gpu_vecchia.py holds cocons_vecchia_predict to on a given table; the
table here is the restatement's, fed with the device's covariance as in test_gpu_corr_knn_pred.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_knn_reference as CR  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_corr_knn_pred import SIZES, _thetas, data, restatement_inputs  # noqa: E402,F401
from test_gpu_dense_sizes import PARITY  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,mp", SIZES)
@pytest.mark.parametrize("which", ["bessel", "closed"])
def test_predict_corr_knn_has_the_bits_of_predict_with_the_exported_table(data, which, n, mp):  # noqa: F811
    import cocons_amd as ca
    th, sl = _thetas()[which]
    th = dict(th, mean=np.array([0.3, -0.2, 0.1]))
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    lp, Xp = data[3][:mp], np.asfortranarray(data[4][:mp])
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        for mc, hops, m in ((5, 2, 5), (30, 2, 30), (60, 1, 30), (1, 1, 1), (63, 2, 63), (5, 1, 3)):
            nn = f.neighbours_corr_pred(th, lp, Xp, m, m_cand=mc, hops=hops)
            want = f.predict_core(th, lp, Xp, nn)
            got = f.predict_corr_knn_core(th, lp, Xp, m, m_cand=mc, hops=hops)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (mc, hops, m)
            assert np.all(np.isfinite(got[0])) and np.all(got[1] >= 0)
    finally:
        f.close()


def test_rows_depend_neither_on_the_chunking_nor_on_the_other_rows(data):  # noqa: F811
    import cocons_amd as ca
    th, sl = _thetas()["bessel"]
    n = 300
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        rows = f.info()["rows"]
        assert rows == 16384
        mp = rows + 3
        reps = mp // 300 + 1
        lp = np.tile(data[3], (reps, 1))[:mp] + np.linspace(0.0, 1e-3, mp)[:, None]
        Xp = np.asfortranarray(np.tile(data[4], (reps, 1))[:mp])
        st, qf = f.predict_corr_knn_core(th, lp, Xp, 5, m_cand=5, hops=2)
        nn = f.neighbours_corr_pred(th, lp, Xp, 5, m_cand=5, hops=2)
        for a, b in ((0, 100), (rows, mp), (rows - 2, rows + 1)):
            s1, q1 = f.predict_corr_knn_core(th, lp[a:b], np.asfortranarray(Xp[a:b]), 5, m_cand=5, hops=2)
            assert np.array_equal(s1, st[a:b]) and np.array_equal(q1, qf[a:b]), (a, b)
            assert np.array_equal(f.neighbours_corr_pred(th, lp[a:b], np.asfortranarray(Xp[a:b]), 5, m_cand=5, hops=2), nn[a:b])
        assert np.all(nn > 0)
    finally:
        f.close()


def test_existing_prediction_entries_keep_their_bits(data):  # noqa: F811
    import cocons_amd as ca
    th, sl = _thetas()["closed"]
    th = dict(th, mean=np.array([0.3, -0.2, 0.1]))
    n, mp = 300, 65
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    lp, Xp = data[3][:mp], np.asfortranarray(data[4][:mp])
    nnp = ca.vecchia_neighbours_pred_device(locs, lp, 12)
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    g = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        before = f.predict_knn_core(th, lp, Xp, 12), f.predict_core(th, lp, Xp, nnp)
        assert all(np.array_equal(u, v) for u, v in zip(before[0], before[1]))
        f.predict_corr_knn_core(th, lp, Xp, 12, m_cand=24, hops=2)
        f.neighbours_corr_pred(th, lp, Xp, 12, m_cand=30, hops=1)
        after = f.predict_knn_core(th, lp, Xp, 12), f.predict_core(th, lp, Xp, nnp)
        for u, v in zip(before, after):
            assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])
        # and a fresh handle that starts with the new entry gives what the old handle gives
        a = g.predict_corr_knn_core(th, lp, Xp, 12, m_cand=24, hops=2)
        b = f.predict_corr_knn_core(th, lp, Xp, 12, m_cand=24, hops=2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c = g.predict_knn_core(th, lp, Xp, 12)
        assert np.array_equal(c[0], before[0][0]) and np.array_equal(c[1], before[0][1])
    finally:
        f.close()
        g.close()


def test_prediction_against_a_numpy_local_kriging_on_the_cpu_oracle(data):  # noqa: F811
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from oracle import oracle as O
    O.build()
    n, mp, m = 700, 50, 30
    th = dict(CR.theta_aniso(5.0), mean=np.array([0.25]))
    sl = wl.SMOOTH_LIMITS
    locs, z, lp = data[0][:n], data[2][:n], data[3][:mp]
    X, Xp = np.ones((n, 1), order="F"), np.ones((mp, 1), order="F")
    S = O.cov_rns(th, locs, X, sl)
    Cp = O.cov_rns_pred(th, locs, lp, X, Xp, sl)
    Cq, dq, d = restatement_inputs(th, sl, locs, X, lp, Xp)
    resid = z - X @ th["mean"]
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        for mc, hops in ((30, 2), (60, 1)):
            nn = ca.vecchia_neighbours_corr_pred(Cq, dq, d, ca.vecchia_neighbours_pred_device(locs, lp, mc),
                                                 ca.vecchia_neighbours_pred_device(locs, locs, mc), m, hops)
            ws, wq = VR.predict(S, Cp, nn, resid)
            gs, gq = f.predict_corr_knn_core(th, lp, Xp, m, m_cand=mc, hops=hops)
            errs = (float(np.max(np.abs(gs - ws)) / np.max(np.abs(ws))), float(np.max(np.abs(gq - wq)) / np.max(np.abs(wq))))
            print("corr-pred-report oracle pin | theta_aniso(5) n%d mp%d m%d m_cand%d hops%d | stochastic %.2e quadform %.2e"
                  % (n, mp, m, mc, hops, errs[0], errs[1]))
            assert max(errs) < PARITY, errs
    finally:
        f.close()


def test_cocopredict_vecchia_corr_knn_is_cocopredict_vecchia_with_the_exported_table(data):  # noqa: F811
    import cocons_amd as ca
    th, sl = _thetas()["bessel"]
    th = dict(th, mean=np.array([0.3, -0.2, 0.1]))
    n, mp = 300, 40
    locs, X, z = data[0][:n], np.asfortranarray(data[1][:n]), data[2][:n]
    lp, Xp = data[3][:mp], np.asfortranarray(data[4][:mp])
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, sl, 5)
    try:
        nn = f.neighbours_corr_pred(th, lp, Xp, 12, m_cand=24, hops=2)
    finally:
        f.close()
    for type_ in ("pred", "mean"):
        want = ca.cocoPredict_vecchia(th, locs, lp, X, Xp, sl, z, nn, type=type_)
        got = ca.cocoPredict_vecchia_corr_knn(th, locs, lp, X, Xp, sl, z, 12, m_cand=24, hops=2, type=type_)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (type_, k)
