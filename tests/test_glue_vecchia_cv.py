"""The U' and cross-validation shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way
tests/test_glue_vecchia_sim.py drives the U^-1 shims: `_cocons_hip_vecchia_transpose`, `_cocons_hip_vecchia_whiten_t` and
`_cocons_hip_vecchia_cv` are registered with their arities, refuse bad arguments as R errors before any device work, and on the
GPU return what the Python layer returns, to the bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_glue_exec import RStub, _problem  # noqa: E402


@pytest.fixture(scope="module")
def R():
    return RStub()


def test_registration_and_refusals_without_a_device(R):
    for name, arity in {"_cocons_hip_vecchia_transpose": 1, "_cocons_hip_vecchia_whiten_t": 3, "_cocons_hip_vecchia_cv": 3}.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    locs, X, th, z = _problem(6)
    n = z.size
    R.L.R_MakeExternalPtr.restype, R.L.R_MakeExternalPtr.argtypes = ctypes.c_void_p, [ctypes.c_void_p] * 3
    closed = R.L.R_MakeExternalPtr(None, R.nil, R.nil)                      # a handle restored from a saved workspace
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_transpose", closed)
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_whiten_t", closed, R.theta(th), R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_cv", closed, R.theta(th, drop_mean=False), R.nil)
    # a handle of n = 36, p = 3, r = 1 whose address is never used: every call below is refused by the shim on its arguments
    fake = R.L.R_MakeExternalPtr(ctypes.c_void_p(1), R.integer([n, 3, 1, 0]), R.nil)
    with pytest.raises(RuntimeError, match="W must be a double matrix with 36 rows"):
        R.call("_cocons_hip_vecchia_whiten_t", fake, R.theta(th), R.real(np.zeros((n - 1, 2))))
    with pytest.raises(RuntimeError, match="W must be a double matrix with 36 rows"):
        R.call("_cocons_hip_vecchia_whiten_t", fake, R.theta(th), R.real(np.zeros(n)))
    with pytest.raises(RuntimeError, match="fold must be NULL or 36 integer labels"):
        R.call("_cocons_hip_vecchia_cv", fake, R.theta(th, drop_mean=False), R.integer(np.zeros(n - 1)))
    with pytest.raises(RuntimeError, match="fold must be NULL or 36 integer labels"):
        R.call("_cocons_hip_vecchia_cv", fake, R.theta(th, drop_mean=False), R.real(np.zeros(n)))
    with pytest.raises(RuntimeError, match="theta has no element 'mean'"):
        R.call("_cocons_hip_vecchia_cv", fake, R.theta(th), R.nil)


@pytest.mark.gpu
def test_the_three_wrappers_equal_the_python_results(R):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n, m = z.size, 12
    rng = np.random.default_rng(12)
    W = rng.standard_normal((n, 2))
    fold = (rng.permutation(n) // 7).astype(np.int32)                     # 28 folds of seven
    h = R.call("_cocons_hip_vecchia_create_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer([m]))
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, m)
    try:
        ptr, rows, info = R.value(R.call("_cocons_hip_vecchia_transpose", h))
        t = f.transpose()
        assert np.array_equal(ptr, t["ptr"]) and np.array_equal(rows, t["rows"])
        assert [int(v) for v in info] == [t["entries"], t["longest"], t["bytes"], t["unnamed"]]
        st, (ut, qd) = R.value(R.call("_cocons_hip_vecchia_whiten_t", h, R.theta(th), R.real(W)))
        want = f.whiten_t_core(th, W)
        assert int(st[0]) == 0 and np.array_equal(ut, want[0]) and np.array_equal(np.ravel(qd), want[1])
        worst = 0.0
        for lab in (None, fold):
            st, (resid, var, stats) = R.value(R.call("_cocons_hip_vecchia_cv", h, R.theta(th, drop_mean=False),
                                                     R.nil if lab is None else R.integer(lab)))
            wr, wv, ws = f.cv_core(th, lab, stats=True)
            assert int(st[0]) == 0 and np.array_equal(np.asarray(resid).reshape(wr.shape), wr) and np.array_equal(np.ravel(var), wv)
            assert [int(v) for v in stats] == [ws["singles"], ws["folds"], ws["entries"], ws["bytes"]]
            worst = max(worst, float(np.max(np.abs(np.asarray(resid).reshape(wr.shape) - wr))))
        print("vecchia-cv-report glue | transpose, whiten_t, leave-one-out and folds through the R wrappers | n%d m%d | worst "
              "deviation %.1e" % (n, m, worst))
        with pytest.raises(RuntimeError, match="cocons_cv_vecchia: fold 0 holds all 196 observations"):
            R.call("_cocons_hip_vecchia_cv", h, R.theta(th, drop_mean=False), R.integer(np.zeros(n)))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
