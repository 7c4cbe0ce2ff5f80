"""The Vecchia handle and local kriging with the neighbours searched on the device (cocons_fit_create_vecchia_knn,
cocons_vecchia_predict_knn) against the same entries fed with the exported table
(cocons_vecchia_neighbours): every output TO THE BIT -- the worst deviation allowed is 0.  Lines "knn-report ..." carry the
cases (tests/golden/VECCHIA_KNN_REPORT.md)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_dense_sizes import problem  # noqa: E402

pytestmark = pytest.mark.gpu


def _report(what, case, dev):
    print("knn-report gpu | %s | %s | worst deviation %.1e" % (what, case, dev))


def _dev(a, b):
    a, b = np.asarray(a, dtype=float).ravel(), np.asarray(b, dtype=float).ravel()
    assert a.shape == b.shape
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return 0.0 if np.all(same) else float(np.max(np.abs(a - b)[~same]))


def _dirs(p):
    return np.random.default_rng(77).standard_normal((3, 6, p))


def _outputs(f, th, Rz, p):
    v, parts = f.neg2loglik_core(th)
    Y, logd = f.whiten_core(th, Rz)
    gv, gparts, gt, gq, gm = f.neg2loglik_grad_core(th)
    info, info_mean = f.fisher_core(th, _dirs(p))
    return {"value": [v], "parts": parts, "whitened": Y, "logd": logd, "grad value": [gv], "grad parts": gparts,
            "grad table": gt, "grad quad": gq, "grad mean": gm, "info": info, "info mean": info_mean}


@pytest.mark.parametrize("m", (1, 30, 63))
@pytest.mark.parametrize("n", (2, 65, 300, 641))
def test_handle_from_knn_has_the_bits_of_the_handle_from_the_exported_table(n, m):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    nn = ca.vecchia_neighbours_device(locs, m)
    a = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, m)
    b = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        assert a.m == b.m == m and a.info()["n"] == n and a.info()["m"] == m
        assert a.info()["bytes"] == b.info()["bytes"]
        oa, ob = _outputs(a, th, Rz, X.shape[1]), _outputs(b, th, Rz, X.shape[1])
    finally:
        a.close()
        b.close()
    worst = max(_dev(oa[k], ob[k]) for k in oa)
    _report("handle: value parts whitened logd gradient information", "n%d m%d" % (n, m), worst)
    for k in oa:
        assert np.array_equal(np.asarray(oa[k]), np.asarray(ob[k]), equal_nan=True), k


def _pred_sites(n, rows):
    """new locations in and around the unit square; row 3 sits exactly on observation 17"""
    locs, X = problem(n)[0], problem(n)[1]
    rng = np.random.default_rng(900 + rows)
    lp = rng.uniform(-0.1, 1.1, size=(rows, 2))
    lp[3] = locs[17]
    Xp = np.asfortranarray(np.column_stack([np.ones(rows)] + [rng.standard_normal(rows) * 0.5 for _ in range(X.shape[1] - 1)]))
    return lp, Xp


@pytest.mark.parametrize("m_pred", (1, 30, 63))
def test_predict_knn_has_the_bits_of_predict_with_the_exported_table(m_pred):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 300
    locs, X, th, z = problem(n)[:4]
    lp, Xp = _pred_sites(n, 70)
    nnp = ca.vecchia_neighbours_pred_device(locs, lp, m_pred)
    assert 18 in nnp[3] and nnp[3, 0] == 18                # the site on observation 17 (1-based 18) has it first: d2 = 0
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, 10)
    try:
        want = f.predict_core(th, lp, Xp, nnp, z_col=1)
        before = f.info()["bytes"]
        got = f.predict_knn_core(th, lp, Xp, m_pred, z_col=1)
        grown = f.info()["bytes"]
        again = f.predict_knn_core(th, lp, Xp, m_pred, z_col=1)
        assert f.info()["bytes"] == grown > before         # the grid: made by the first call, kept
        halves = [f.predict_knn_core(th, lp[a:b], Xp[a:b], m_pred, z_col=1) for a, b in ((0, 35), (35, 70))]
    finally:
        f.close()
    worst = max(_dev(got[0], want[0]), _dev(got[1], want[1]))
    _report("prediction: stochastic quadform", "n%d m_pred%d rows 70, twice, in two halves" % (n, m_pred), worst)
    for k in (0, 1):
        assert np.array_equal(got[k], want[k]) and np.array_equal(again[k], want[k])
        assert np.array_equal(np.concatenate([h[k] for h in halves]), want[k])
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))


def test_predict_knn_over_more_rows_than_a_chunk():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, mp, m_pred = 300, 20000, 30
    locs, X, th, z = problem(n)[:4]
    lp, Xp = _pred_sites(n, mp)
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, 10)
    try:
        assert mp > f.info()["rows"]
        want = f.predict_core(th, lp, Xp, ca.vecchia_neighbours_pred_device(locs, lp, m_pred))
        got = f.predict_knn_core(th, lp, Xp, m_pred)
        tail = f.predict_knn_core(th, lp[-50:], Xp[-50:], m_pred)       # rows of the second chunk, alone
    finally:
        f.close()
    _report("prediction: stochastic quadform", "n%d m_pred%d rows %d (two chunks)" % (n, m_pred, mp),
            max(_dev(got[0], want[0]), _dev(got[1], want[1])))
    for k in (0, 1):
        assert np.array_equal(got[k], want[k]) and np.array_equal(tail[k], want[k][-50:])


def test_predict_knn_with_more_neighbours_than_observations():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m_pred = 65, 30
    locs, X, th, z = problem(n)[:4]
    k = 12                                                  # a handle over the first 12 observations: m_pred > n
    lp, Xp = _pred_sites(n, 40)
    f = ca.CoconsVecchiaFit.from_knn(locs[:k], X[:k], z[:k], wl.SMOOTH_LIMITS, 5)
    try:
        nnp = ca.vecchia_neighbours_pred_device(locs[:k], lp, m_pred)
        assert np.all(nnp[:, k:] == 0) and np.all(np.sort(nnp[:, :k], axis=1) == np.arange(1, k + 1))
        want = f.predict_core(th, lp, Xp, nnp)
        got = f.predict_knn_core(th, lp, Xp, m_pred)
    finally:
        f.close()
    _report("prediction: stochastic quadform", "n%d m_pred%d (zero-padded rows)" % (k, m_pred),
            max(_dev(got[0], want[0]), _dev(got[1], want[1])))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_other_kinds_of_handle_are_refused_by_name_and_keep_their_bits():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n = 65
    locs, X, th, z = problem(n)[:4]
    lp, Xp = _pred_sites(n, 40)
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    taper = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, 0.2)
    try:
        before = dense.neg2loglik_core(th)
        st, qf = np.full(40, 7.0), np.full(40, 7.0)
        for h in (dense, taper):
            rc = h._L.cocons_vecchia_predict_knn(h._h, host._p(T), host._p(mean), 0, 40, host._p(np.asfortranarray(lp)),
                                                 host._p(Xp), 10, host._p(st), host._p(qf))
            assert rc == -1
            assert _lib.last_error() == "cocons_vecchia_predict_knn: not a Vecchia fit (cocons_fit_create_vecchia makes one)"
        assert np.all(st == 7.0) and np.all(qf == 7.0)
        f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, 10)
        try:
            f.neg2loglik_core(th)
            f.predict_knn_core(th, lp, Xp, 10)
            with pytest.raises(_lib.CoconsHipError, match="z_col = 5 is outside"):
                f.predict_knn_core(th, lp, Xp, 10, z_col=5)
            val, parts = ctypes.c_double(0.0), np.zeros(1 + z.shape[1])
            assert f._L.cocons_neg2loglik_dense(f._h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts)) < 0
            assert _lib.last_error().startswith("cocons_neg2loglik_dense: not available on a Vecchia fit")
        finally:
            f.close()
        ca.vecchia_neighbours_device(locs, 10)
        after = dense.neg2loglik_core(th)
    finally:
        dense.close()
        taper.close()
    assert before[0] == after[0] and np.array_equal(before[1], after[1])


def test_cocopredict_vecchia_knn_is_cocopredict_vecchia_with_the_exported_table():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 300
    locs, X, th, z = problem(n)[:4]
    lp, Xp = _pred_sites(n, 70)
    nnp = ca.vecchia_neighbours_pred_device(locs, lp, 20)
    want = ca.cocoPredict_vecchia(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, nnp)
    got = ca.cocoPredict_vecchia_knn(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, 20)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
