"""The neighbour-search shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way
tests/test_glue_vecchia.py drives the other Vecchia shims: `_cocons_hip_vecchia_neighbours`, `_cocons_hip_vecchia_create_knn`
and `_cocons_hip_vecchia_predict_knn` are registered with their arities, refuse bad arguments as R errors before any device
work, and on the GPU return what the Python layer returns, to the bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_glue_exec import RStub, _problem  # noqa: E402


@pytest.fixture(scope="module")
def R():
    return RStub()


def _int_matrix(R, s):
    return R.value(s).reshape((R.L.stub_nrow(s), R.L.stub_ncol(s)), order="F")


def test_registration_and_refusals_without_a_device(R):
    from cocons_amd import workloads as wl
    for name, arity in {"_cocons_hip_vecchia_neighbours": 4, "_cocons_hip_vecchia_create_knn": 6,
                        "_cocons_hip_vecchia_predict_knn": 6}.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    locs, X, th, z = _problem(6)
    n = z.size
    z = z.reshape(n, 1)
    bad = np.array(locs)
    bad[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="cocons_vecchia_neighbours: m = 64 is outside 1 .. 63"):
        R.call("_cocons_hip_vecchia_neighbours", R.real(locs), R.nil, R.integer([64]), R.integer([0]))
    with pytest.raises(RuntimeError, match="cocons_vecchia_neighbours: a coordinate of locs is not finite"):
        R.call("_cocons_hip_vecchia_neighbours", R.real(bad), R.nil, R.integer([5]), R.integer([0]))
    with pytest.raises(RuntimeError, match="cocons_vecchia_neighbours: a coordinate of locs_query is not finite"):
        R.call("_cocons_hip_vecchia_neighbours", R.real(locs), R.real(bad[:7]), R.integer([5]), R.integer([0]))
    with pytest.raises(RuntimeError, match="locs must be a double matrix with 2 columns"):
        R.call("_cocons_hip_vecchia_neighbours", R.real(locs[:, 0]), R.nil, R.integer([5]), R.integer([0]))
    for m, text in ((0, "m = 0 is outside 1 .. 63"), (64, "m = 64 is outside 1 .. 63")):
        with pytest.raises(RuntimeError, match="cocons_fit_create_vecchia_knn: " + text):
            R.call("_cocons_hip_vecchia_create_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
                   R.integer([0]), R.integer([m]))
    with pytest.raises(RuntimeError, match="cocons_fit_create_vecchia_knn: a coordinate of locs is not finite"):
        R.call("_cocons_hip_vecchia_create_knn", R.real(bad), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer([5]))


@pytest.mark.gpu
def test_the_three_wrappers_equal_the_python_results(R):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    m, m_pred = 12, 9
    lp = locs[:21] + 0.013
    lp[5] = locs[9]                                                       # on an observation
    Xp = np.asfortranarray(X[:21] * 0.9)
    # the tables
    nn = _int_matrix(R, R.call("_cocons_hip_vecchia_neighbours", R.real(locs), R.nil, R.integer([m]), R.integer([0])))
    assert np.array_equal(nn, ca.vecchia_neighbours_device(locs, m))
    nnp = _int_matrix(R, R.call("_cocons_hip_vecchia_neighbours", R.real(locs), R.real(lp), R.integer([m_pred]), R.integer([0])))
    assert np.array_equal(nnp, ca.vecchia_neighbours_pred_device(locs, lp, m_pred)) and nnp[5, 0] == 10
    # the handle and the prediction
    h = R.call("_cocons_hip_vecchia_create_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer([m]))
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, m)
    try:
        st, v = R.value(R.call("_cocons_hip_vecchia_neg2loglik", h, R.theta(th), R.real(th["mean"])))
        val, parts = f.neg2loglik_core(th)
        assert int(st[0]) == 0 and v[0] == val and np.array_equal(v[1:], parts)
        st, kr = R.value(R.call("_cocons_hip_vecchia_predict_knn", h, R.theta(th, drop_mean=False), R.integer([1]), R.real(lp),
                                R.real(Xp), R.integer([m_pred])))
        ws, wq = f.predict_knn_core(th, lp, Xp, m_pred)
        assert int(st[0]) == 0 and kr.shape == (21, 2)
        assert np.array_equal(kr[:, 0], ws) and np.array_equal(kr[:, 1], wq)
        print("knn-report glue | tables value prediction through the R wrappers | n%d m%d m_pred%d | worst deviation %.1e"
              % (z.size, m, m_pred, max(float(np.max(np.abs(kr[:, 0] - ws))), float(np.max(np.abs(kr[:, 1] - wq))))))
        with pytest.raises(RuntimeError, match="cocons_vecchia_predict_knn: m_pred = 64 is outside 1 .. 63"):
            R.call("_cocons_hip_vecchia_predict_knn", h, R.theta(th, drop_mean=False), R.integer([1]), R.real(lp), R.real(Xp),
                   R.integer([64]))
        with pytest.raises(RuntimeError, match="theta has no element 'mean'"):
            R.call("_cocons_hip_vecchia_predict_knn", h, R.theta(th), R.integer([1]), R.real(lp), R.real(Xp), R.integer([m_pred]))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
