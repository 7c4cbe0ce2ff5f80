"""The shims of the neighbours of new locations by model correlation and of the grouped handle on a correlation table
 in glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way tests/test_glue_vecchia_corr.py drives
the observations': `_cocons_hip_vecchia_neighbours_corr_pred`, `_cocons_hip_vecchia_predict_corr_knn` and
`_cocons_hip_vecchia_create_grouped_corr_knn` are registered with their arities, the R wrappers call them, bad arguments are R
errors before any device work, and on the GPU they return what the Python layer returns, to the bit."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_glue_exec import ROOT, RStub, _problem  # noqa: E402


@pytest.fixture(scope="module")
def R():
    return RStub()


def _create(R, locs, X, z, th, m_cand, hops, m, max_rows=64, max_rounds=0):
    from cocons_amd import workloads as wl
    return R.call("_cocons_hip_vecchia_create_grouped_corr_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
                  R.integer([0]), R.theta(th), R.integer([m_cand, hops, m]), R.integer([max_rows]), R.integer([max_rounds]))


def test_registration_wrappers_and_refusals_without_a_device(R):
    for name, arity in {"_cocons_hip_vecchia_neighbours_corr_pred": 5, "_cocons_hip_vecchia_predict_corr_knn": 6,
                        "_cocons_hip_vecchia_create_grouped_corr_knn": 9}.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry in ((r"\.cocons\.hip\.vecchia\.neighbours\.corr\.pred", "_cocons_hip_vecchia_neighbours_corr_pred"),
                      (r"\.cocons\.hip\.vecchia\.predict\.corr\.knn", "_cocons_hip_vecchia_predict_corr_knn"),
                      (r"\.cocons\.hip\.vecchia\.create\.grouped\.corr\.knn", "_cocons_hip_vecchia_create_grouped_corr_knn")):
        m = re.search(fn + r" <- function\((.*?)\) \{(.*?)\n\}", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
    locs, X, th, z = _problem(6)
    z = z.reshape(-1, 1)
    bad = np.array(locs)
    bad[3, 1] = np.nan
    who = "cocons_fit_create_vecchia_grouped_corr_knn: "
    for (mc, hops, m), text in (((0, 2, 3), "m_cand = 0 is outside 1 .. 63"), ((64, 2, 3), "m_cand = 64 is outside 1 .. 63"),
                                ((5, 0, 3), "hops = 0 is outside 1 .. 2"), ((5, 3, 3), "hops = 3 is outside 1 .. 2"),
                                ((5, 2, 0), "m = 0 is outside 1 .. 63"), ((5, 2, 64), "m = 64 is outside 1 .. 63"),
                                ((5, 1, 6), "m = 6, but a row has 5 candidates at the most")):
        with pytest.raises(RuntimeError, match=re.escape(who + text)):
            _create(R, locs, X, z, th, mc, hops, m)
    with pytest.raises(RuntimeError, match=re.escape(who + "max_rows = 1 is outside 2 .. ")):
        _create(R, locs, X, z, th, 5, 2, 3, max_rows=1)
    with pytest.raises(RuntimeError, match=re.escape(who + "max_rounds = -1")):
        _create(R, locs, X, z, th, 5, 2, 3, max_rounds=-1)
    with pytest.raises(RuntimeError, match=who + "a coordinate of locs is not finite"):
        _create(R, bad, X, z, th, 5, 2, 3)
    nan_th = {k: np.array(v, dtype=float) for k, v in th.items()}
    nan_th["tilt"][1] = np.nan
    with pytest.raises(RuntimeError, match=who + r"theta\[10\] is not finite"):
        _create(R, locs, X, z, nan_th, 5, 2, 3)
    with pytest.raises(RuntimeError, match="theta has no element 'aniso'"):
        _create(R, locs, X, z, {k: v for k, v in th.items() if k != "aniso"}, 5, 2, 3)
    with pytest.raises(RuntimeError, match="locs must be n x 2"):
        _create(R, locs[:-1], X, z, th, 5, 2, 3)


@pytest.mark.gpu
def test_the_three_wrappers_equal_the_python_results(R):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    lp, Xp = np.asfortranarray(locs[:21] + 0.013), np.asfortranarray(X[:21] * 0.9)
    lp[5] = locs[9]
    m_cand, hops, m = 9, 2, 12
    h = _create(R, locs, X, z, th, m_cand, hops, m, max_rows=17)
    f = ca.CoconsVecchiaFit.from_groups_corr_knn(locs, X, z, wl.SMOOTH_LIMITS, th, m, m_cand=m_cand, hops=hops, max_rows=17)
    try:
        st, v = R.value(R.call("_cocons_hip_vecchia_neg2loglik", h, R.theta(th), R.real(th["mean"])))
        val, parts = f.neg2loglik_core(th)
        assert int(st[0]) == 0 and v[0] == val and np.array_equal(v[1:], parts)
        st, nn = R.value(R.call("_cocons_hip_vecchia_neighbours_corr_pred", h, R.theta(th), R.real(lp), R.real(Xp),
                                R.integer([m_cand, hops, m])))
        want = f.neighbours_corr_pred(th, lp, Xp, m, m_cand=m_cand, hops=hops)
        assert int(st[0]) == 0 and np.array_equal(nn.reshape(want.shape, order="F"), want) and np.all(want > 0)
        assert want[5, 0] == 10
        st, kr = R.value(R.call("_cocons_hip_vecchia_predict_corr_knn", h, R.theta(th, drop_mean=False), R.integer([1]), R.real(lp),
                                R.real(Xp), R.integer([m_cand, hops, m])))
        gs, gq = f.predict_corr_knn_core(th, lp, Xp, m, m_cand=m_cand, hops=hops)
        kr = kr.reshape((21, 2), order="F")
        assert int(st[0]) == 0 and np.array_equal(kr[:, 0], gs) and np.array_equal(kr[:, 1], gq)
        for args, text in (((64, 2, 3), "m_cand = 64 is outside 1 .. 63"), ((5, 3, 3), "hops = 3 is outside 1 .. 2"),
                           ((5, 1, 6), "m = 6, but a row has 5 candidates at the most")):
            with pytest.raises(RuntimeError, match=re.escape("cocons_vecchia_neighbours_corr_pred: " + text)):
                R.call("_cocons_hip_vecchia_neighbours_corr_pred", h, R.theta(th), R.real(lp), R.real(Xp), R.integer(list(args)))
            with pytest.raises(RuntimeError, match=re.escape("cocons_vecchia_predict_corr_knn: " + text)):
                R.call("_cocons_hip_vecchia_predict_corr_knn", h, R.theta(th, drop_mean=False), R.integer([1]), R.real(lp),
                       R.real(Xp), R.integer(list(args)))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
