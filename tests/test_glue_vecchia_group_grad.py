"""The grouped-gradient shim of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way
tests/test_glue_vecchia_group.py drives the grouped value shims: `_cocons_hip_vecchia_neg2loglik_grad_grouped` is registered
with its arity, named by its R wrapper, refuses bad arguments as R errors before any device work, and on the GPU returns what
the Python core returns, to the bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_glue_exec import ROOT, RStub, _problem  # noqa: E402

SHIM = "_cocons_hip_vecchia_neg2loglik_grad_grouped"


@pytest.fixture(scope="module")
def R():
    return RStub()


def test_registration_and_refusals_without_a_device(R):
    assert R.L.stub_registered_arity(SHIM.encode()) == 3
    rfile = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    body = rfile[rfile.index(".cocons.hip.vecchia.neg2loglik.grad.grouped <- function"):]
    assert "`%s`" % SHIM in body[:body.index("\n}\n")]
    th = _problem(8)[2]
    R.L.R_MakeExternalPtr.restype, R.L.R_MakeExternalPtr.argtypes = ctypes.c_void_p, [ctypes.c_void_p] * 3
    closed = R.L.R_MakeExternalPtr(None, R.nil, R.nil)                      # a handle restored from a saved workspace
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call(SHIM, closed, R.theta(th), R.real(th["mean"]))
    fake = R.L.R_MakeExternalPtr(ctypes.c_void_p(1), R.integer([64, 3, 1, 0]), R.nil)     # its address is never used
    with pytest.raises(RuntimeError, match="mean must have length 3"):
        R.call(SHIM, fake, R.theta(th), R.real(np.zeros(2)))


@pytest.mark.gpu
def test_the_wrapper_equals_the_python_core(R):
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n, m = z.size, 12
    nn = host.vecchia_neighbours(locs, m)
    group = R.value(R.call("_cocons_hip_vecchia_group", R.real(nn.astype(float)), R.integer([64])))[0]
    wide = np.asarray(R.value(R.call("_cocons_hip_vecchia_group_table", R.real(nn.astype(float)), R.integer(group)))).reshape((n, -1), order="F")
    h = R.call("_cocons_hip_vecchia_create", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)), R.integer([0]),
               R.real(wide.astype(float)))
    f = ca.CoconsVecchiaFit.from_groups(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        with pytest.raises(RuntimeError, match="cocons_neg2loglik_grad_vecchia_grouped: the handle has no plan"):
            R.call(SHIM, h, R.theta(th), R.real(th["mean"]))
        R.call("_cocons_hip_vecchia_set_groups", h, R.integer(group))
        st, res = R.value(R.call(SHIM, h, R.theta(th), R.real(th["mean"])))
        val, _, gt, gq, gm = f.neg2loglik_grad_core(th, grouped=True)
        assert int(st[0]) == 0 and float(np.ravel(res[0])[0]) == val
        assert res[1].shape == (6, gm.size) and np.array_equal(res[1], gt) and np.array_equal(res[2], gq)
        assert np.array_equal(np.ravel(res[3]), gm)
        print("vecchia-group-grad-report glue | value, table, quad and mean through the R wrapper | n%d m%d | %.1e" % (n, m, 0.0))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
