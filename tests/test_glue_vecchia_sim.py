"""The U^-1 shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way tests/test_glue_vecchia_knn.py
drives the neighbour-search shims: `_cocons_hip_vecchia_unwhiten`, `_cocons_hip_vecchia_sim` and `_cocons_hip_vecchia_schedule`
are registered with their arities, refuse bad arguments as R errors before any device work, and on the GPU return what the
Python layer returns, to the bit."""
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
    for name, arity in {"_cocons_hip_vecchia_unwhiten": 3, "_cocons_hip_vecchia_sim": 5, "_cocons_hip_vecchia_schedule": 2}.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    locs, X, th, z = _problem(6)
    n = z.size
    R.L.R_MakeExternalPtr.restype, R.L.R_MakeExternalPtr.argtypes = ctypes.c_void_p, [ctypes.c_void_p] * 3
    closed = R.L.R_MakeExternalPtr(None, R.nil, R.nil)                      # a handle restored from a saved workspace
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_unwhiten", closed, R.theta(th), R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_sim", closed, R.theta(th, drop_mean=False), R.integer([0]), R.integer([1]),
               R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_schedule", closed, R.integer([0]))
    # a handle of n = 36, p = 3, r = 1 whose address is never used: every call below is refused by the shim on its arguments
    fake = R.L.R_MakeExternalPtr(ctypes.c_void_p(1), R.integer([n, 3, 1, 0]), R.nil)
    with pytest.raises(RuntimeError, match="W must be a double matrix with 36 rows"):
        R.call("_cocons_hip_vecchia_unwhiten", fake, R.theta(th), R.real(np.zeros((n - 1, 2))))
    with pytest.raises(RuntimeError, match="W must be a double matrix with 36 rows"):
        R.call("_cocons_hip_vecchia_unwhiten", fake, R.theta(th), R.real(np.zeros(n)))
    for nf in (-1, n, n + 3):
        with pytest.raises(RuntimeError, match="cocons_sim_vecchia: n_fixed = %d is outside 0 .. 35" % nf):
            R.call("_cocons_hip_vecchia_sim", fake, R.theta(th, drop_mean=False), R.integer([nf]), R.integer([1]),
                   R.real(np.zeros((n, 1))))
        with pytest.raises(RuntimeError, match="cocons_vecchia_schedule: n_fixed = %d is outside 0 .. 35" % nf):
            R.call("_cocons_hip_vecchia_schedule", fake, R.integer([nf]))
    with pytest.raises(RuntimeError, match="iiderrors must be a double matrix with 26 rows"):
        R.call("_cocons_hip_vecchia_sim", fake, R.theta(th, drop_mean=False), R.integer([10]), R.integer([1]),
               R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="theta has no element 'mean'"):
        R.call("_cocons_hip_vecchia_sim", fake, R.theta(th), R.integer([10]), R.integer([1]), R.real(np.zeros((n - 10, 1))))


@pytest.mark.gpu
def test_the_three_wrappers_equal_the_python_results(R):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n, m, nf = z.size, 12, 150
    rng = np.random.default_rng(12)
    W, E = rng.standard_normal((n, 2)), rng.standard_normal((n - nf, 3))
    h = R.call("_cocons_hip_vecchia_create_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer([m]))
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, m)
    try:
        st, x = R.value(R.call("_cocons_hip_vecchia_unwhiten", h, R.theta(th), R.real(W)))
        assert int(st[0]) == 0 and np.array_equal(x, f.unwhiten_core(th, W))
        st, y = R.value(R.call("_cocons_hip_vecchia_sim", h, R.theta(th, drop_mean=False), R.integer([0]), R.integer([1]), R.real(W)))
        assert int(st[0]) == 0 and np.array_equal(y, f.sim_core(th, W))
        st, c = R.value(R.call("_cocons_hip_vecchia_sim", h, R.theta(th, drop_mean=False), R.integer([nf]), R.integer([1]), R.real(E)))
        want = f.sim_core(th, E, n_fixed=nf)
        assert int(st[0]) == 0 and c.shape == (n - nf, 3) and np.array_equal(c, want)
        for k in (0, nf):
            lv, info = R.value(R.call("_cocons_hip_vecchia_schedule", h, R.integer([k])))
            s = f.schedule(k)
            assert np.array_equal(lv, s["levels"])
            assert [int(v) for v in info] == [s["depth"], s["widest"], s["launches"], s["bytes"]]
        print("vecchia-sim-report glue | unwhiten, sim, conditional sim, schedule through the R wrappers | n%d m%d | worst "
              "deviation %.1e" % (n, m, float(np.max(np.abs(c - want)))))
        with pytest.raises(RuntimeError, match="cocons_sim_vecchia: z_col = 1 is outside 0 .. 0"):
            R.call("_cocons_hip_vecchia_sim", h, R.theta(th, drop_mean=False), R.integer([0]), R.integer([2]), R.real(W))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
