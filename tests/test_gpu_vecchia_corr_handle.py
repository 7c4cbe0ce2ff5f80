"""cocons_fit_create_vecchia_corr_knn: the handle whose table is searched, re-ranked by model correlation and
adopted on the device gives, in every Vecchia entry, the bits of cocons_fit_create_vecchia fed with the exported table -- the
value, the gradient, the whitening, one column of its inverse and leave-one-out cross-validation, at n = 300 and 700 --; its
bytes are those of the handle made from the table; and from_maxmin_corr is from_corr_knn on the rows in the maxmin order, with
per-row arrays carried there and back."""
import numpy as np
import pytest

import corr_knn_reference as CR

pytestmark = pytest.mark.gpu


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _problem(n):
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(20260322 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(wl.design_from_locs(locs)["std.covs"])
    th = CR.theta_covariate()
    th["mean"] = np.array([0.2, -0.1, 0.05])
    return locs, X, rng.standard_normal((n, 2)), th, wl.SMOOTH_LIMITS


@pytest.mark.parametrize("n,m_cand,hops,m", [(300, 20, 2, 10), (700, 30, 2, 30), (300, 40, 1, 20)])
def test_handle_gives_the_bits_of_the_handle_of_the_exported_table(n, m_cand, hops, m):
    import cocons_amd as ca
    locs, X, z, th, sl = _problem(n)
    rng = np.random.default_rng(9)
    B = np.asfortranarray(rng.standard_normal((n, 3)))
    W = np.asfortranarray(rng.standard_normal((n, 1)))
    a = ca.CoconsVecchiaFit.from_corr_knn(locs, X, z, sl, th, m, m_cand=m_cand, hops=hops)
    try:
        nn = a.neighbours_corr(th, m, m_cand=m_cand, hops=hops)
        assert np.any(nn[:, m - 1] > 0) and np.all(nn < np.arange(1, n + 1)[:, None])
        b = ca.CoconsVecchiaFit(locs, X, z, sl, nn)
        try:
            ia, ib = a.info(), b.info()
            assert ia == ib and ia["m"] == m and ia["n"] == n and ia["bytes"] >= n * m * 4, (ia, ib)
            # at another theta than the table's as well: the table is the handle's, whatever is evaluated on it
            other = dict(th, scale=th["scale"] + np.array([0.1, -0.05, 0.0]))
            for t in (th, other):
                assert _same(a.neg2loglik_core(t), b.neg2loglik_core(t))
                assert _same(a.neg2loglik_grad_core(t), b.neg2loglik_grad_core(t))
                assert _same(a.whiten_core(t, B), b.whiten_core(t, B))
                assert _same(a.unwhiten_core(t, W), b.unwhiten_core(t, W))
                assert _same(a.cv_core(t), b.cv_core(t))
            assert a.info() == b.info()
            print("corr-report gpu | from_corr_knn against the handle of the exported table: value gradient whitened unwhitened "
                  "leave-one-out, two thetas | n%d m_cand%d hops%d m%d | %d bytes held | values that differ 0"
                  % (n, m_cand, hops, m, ia["bytes"]))
        finally:
            b.close()
    finally:
        a.close()


def test_from_maxmin_corr_is_from_corr_knn_on_the_permuted_rows():
    import cocons_amd as ca
    n, m = 300, 12
    locs, X, z, th, sl = _problem(n)
    f = ca.CoconsVecchiaFit.from_maxmin_corr(locs, X, z, sl, th, m)
    try:
        o = f.maxmin_order.astype(np.int64) - 1
        assert np.array_equal(np.sort(o), np.arange(n)) and np.array_equal(f.maxmin_order, ca.vecchia_order_device(locs))
        rows = np.arange(n)
        assert np.array_equal(f.to_maxmin(rows), o) and np.array_equal(f.from_maxmin_order(f.to_maxmin(rows)), rows)
        g = ca.CoconsVecchiaFit.from_corr_knn(locs[o], X[o], z[o], sl, th, m)
        try:
            assert _same(f.neg2loglik_core(th), g.neg2loglik_core(th))
            assert np.array_equal(f.neighbours_corr(th, m), g.neighbours_corr(th, m))
            B = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 2)))
            wf = f.whiten_core(th, f.to_maxmin(B))
            assert _same(wf, g.whiten_core(th, B[o]))
            back = f.from_maxmin_order(np.asarray(wf[0] if isinstance(wf, tuple) else wf))
            assert back.shape == (n, 2) and np.array_equal(back[o], np.asarray(wf[0] if isinstance(wf, tuple) else wf))
            print("corr-report gpu | from_maxmin_corr against from_corr_knn on the permuted arrays: value table whitened, round trip "
                  "| n%d m%d | values that differ 0" % (n, m))
        finally:
            g.close()
    finally:
        f.close()
