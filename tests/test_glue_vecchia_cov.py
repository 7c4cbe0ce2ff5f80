"""The U^-T shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way tests/test_glue_vecchia_sim.py drives
the U^-1 shims: `_cocons_hip_vecchia_unwhiten_t`, `_cocons_hip_vecchia_cov_mult`, `_cocons_hip_vecchia_cov_cols` and
`_cocons_hip_vecchia_schedule_t` are registered with their arities, refuse bad arguments as R errors before any device work, and
on the GPU return what the Python layer returns, to the bit."""
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
    for name, arity in {"_cocons_hip_vecchia_unwhiten_t": 4, "_cocons_hip_vecchia_cov_mult": 5, "_cocons_hip_vecchia_cov_cols": 5,
                        "_cocons_hip_vecchia_schedule_t": 2}.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    locs, X, th, z = _problem(6)
    n = z.size
    R.L.R_MakeExternalPtr.restype, R.L.R_MakeExternalPtr.argtypes = ctypes.c_void_p, [ctypes.c_void_p] * 3
    closed = R.L.R_MakeExternalPtr(None, R.nil, R.nil)                      # a handle restored from a saved workspace
    zero = R.integer([0])
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_unwhiten_t", closed, R.theta(th), R.real(np.zeros((n, 1))), zero)
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_cov_mult", closed, R.theta(th), R.real(np.zeros((n, 1))), zero, zero)
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_cov_cols", closed, R.theta(th), R.integer([1]), zero, zero)
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_schedule_t", closed, zero)
    # a handle of n = 36, p = 3, r = 1 whose address is never used: every call below is refused by the shim on its arguments
    fake = R.L.R_MakeExternalPtr(ctypes.c_void_p(1), R.integer([n, 3, 1, 0]), R.nil)
    with pytest.raises(RuntimeError, match="W must be a double matrix with 36 rows"):
        R.call("_cocons_hip_vecchia_unwhiten_t", fake, R.theta(th), R.real(np.zeros((n - 1, 2))), zero)
    with pytest.raises(RuntimeError, match="B must be a double matrix with 26 rows"):
        R.call("_cocons_hip_vecchia_cov_mult", fake, R.theta(th), R.real(np.zeros((n, 2))), R.integer([10]), zero)
    for nf in (-1, n, n + 3):
        with pytest.raises(RuntimeError, match="cocons_vecchia_cov_mult: n_fixed = %d is outside 0 .. 35" % nf):
            R.call("_cocons_hip_vecchia_cov_mult", fake, R.theta(th), R.real(np.zeros((n, 1))), R.integer([nf]), zero)
        with pytest.raises(RuntimeError, match="cocons_vecchia_cov_cols: n_fixed = %d is outside 0 .. 35" % nf):
            R.call("_cocons_hip_vecchia_cov_cols", fake, R.theta(th), R.integer([n]), R.integer([nf]), zero)
        with pytest.raises(RuntimeError, match="cocons_vecchia_schedule_t: n_fixed = %d is outside 0 .. 35" % nf):
            R.call("_cocons_hip_vecchia_schedule_t", fake, R.integer([nf]))
    for bad, at in (([0], 1), ([15, n + 1], 2), ([10], 1)):
        with pytest.raises(RuntimeError, match=r"cocons_vecchia_cov_cols: idx\[%d\] = %d is outside 11 .. 36" % (at, bad[at - 1])):
            R.call("_cocons_hip_vecchia_cov_cols", fake, R.theta(th), R.integer(bad), R.integer([10]), zero)
    with pytest.raises(RuntimeError, match="idx must be an integer vector"):
        R.call("_cocons_hip_vecchia_cov_cols", fake, R.theta(th), R.real(np.ones(2)), zero, zero)


@pytest.mark.gpu
def test_the_four_wrappers_equal_the_python_results(R):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n, m, nf = z.size, 12, 150
    rng = np.random.default_rng(13)
    W, B = rng.standard_normal((n, 2)), rng.standard_normal((n - nf, 3))
    zero = R.integer([0])
    h = R.call("_cocons_hip_vecchia_create_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer([m]))
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, m)
    try:
        st, v = R.value(R.call("_cocons_hip_vecchia_unwhiten_t", h, R.theta(th), R.real(W), zero))
        assert int(st[0]) == 0 and np.array_equal(v, f.unwhiten_t_core(th, W))
        st, a = R.value(R.call("_cocons_hip_vecchia_cov_mult", h, R.theta(th), R.real(W), zero, zero))
        assert int(st[0]) == 0 and np.array_equal(a, f.cov_mult_core(th, W))
        st, b = R.value(R.call("_cocons_hip_vecchia_cov_mult", h, R.theta(th), R.real(B), R.integer([nf]), zero))
        want = f.cov_mult_core(th, B, n_fixed=nf)
        assert int(st[0]) == 0 and b.shape == (n - nf, 3) and np.array_equal(b, want)
        idx = [n, nf + 1, n]
        st, c = R.value(R.call("_cocons_hip_vecchia_cov_cols", h, R.theta(th), R.integer(idx), R.integer([nf]), zero))
        assert int(st[0]) == 0 and c.shape == (n - nf, 3) and np.array_equal(c, f.cov_cols_core(th, idx, n_fixed=nf))
        for k in (0, nf):
            lv, info = R.value(R.call("_cocons_hip_vecchia_schedule_t", h, R.integer([k])))
            s = f.schedule_t(k)
            assert np.array_equal(lv, s["levels"])
            assert [int(x) for x in info] == [s["depth"], s["widest"], s["launches"], s["bytes"]]
        print("vecchia-cov-report glue | unwhiten_t, cov_mult, cov_cols, schedule_t through the R wrappers | n%d m%d | worst "
              "deviation %.1e" % (n, m, float(np.max(np.abs(b - want)))))
        # grouped = 1 on a handle without a plan is the library's refusal, as an R error under the entry's name
        with pytest.raises(RuntimeError, match="cocons_vecchia_unwhiten_t:"):
            R.call("_cocons_hip_vecchia_unwhiten_t", h, R.theta(th), R.real(W), R.integer([1]))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
