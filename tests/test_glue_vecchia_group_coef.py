"""The four grouped coefficient shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way
tests/test_glue_vecchia_group_fisher.py drives the grouped information shim: `_cocons_hip_vecchia_unwhiten_grouped`,
`_cocons_hip_vecchia_sim_grouped`, `_cocons_hip_vecchia_whiten_t_grouped` and `_cocons_hip_vecchia_cv_grouped` are registered
with their twins' arities, refuse bad arguments as R errors before any device work (the twins' code), and on the GPU return what
the C entries return through the Python core, to the bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_glue_exec import RStub, _problem  # noqa: E402

SHIMS = {"unwhiten": 3, "sim": 5, "whiten_t": 3, "cv": 3}


def _shim(name):
    return "_cocons_hip_vecchia_%s_grouped" % name


@pytest.fixture(scope="module")
def R():
    return RStub()


def test_registration_and_refusals_without_a_device(R):
    for name, arity in SHIMS.items():
        assert R.L.stub_registered_arity(_shim(name).encode()) == arity
    n = 36
    th = _problem(6)[2]
    R.L.R_MakeExternalPtr.restype, R.L.R_MakeExternalPtr.argtypes = ctypes.c_void_p, [ctypes.c_void_p] * 3
    closed = R.L.R_MakeExternalPtr(None, R.nil, R.nil)                      # a handle restored from a saved workspace
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call(_shim("unwhiten"), closed, R.theta(th), R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call(_shim("sim"), closed, R.theta(th, drop_mean=False), R.integer([0]), R.integer([1]), R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call(_shim("whiten_t"), closed, R.theta(th), R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call(_shim("cv"), closed, R.theta(th, drop_mean=False), R.nil)
    fake = R.L.R_MakeExternalPtr(ctypes.c_void_p(1), R.integer([n, 3, 1, 0]), R.nil)      # its address is never used
    for name in ("unwhiten", "whiten_t"):
        with pytest.raises(RuntimeError, match="W must be a double matrix with 36 rows"):
            R.call(_shim(name), fake, R.theta(th), R.real(np.zeros((n - 1, 2))))
    with pytest.raises(RuntimeError, match="cocons_sim_vecchia: n_fixed = 36 is outside 0 .. 35"):
        R.call(_shim("sim"), fake, R.theta(th, drop_mean=False), R.integer([n]), R.integer([1]), R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="iiderrors must be a double matrix with 26 rows"):
        R.call(_shim("sim"), fake, R.theta(th, drop_mean=False), R.integer([10]), R.integer([1]), R.real(np.zeros((n, 1))))
    with pytest.raises(RuntimeError, match="fold must be NULL or 36 integer labels"):
        R.call(_shim("cv"), fake, R.theta(th, drop_mean=False), R.integer(np.zeros(n - 1)))
    with pytest.raises(RuntimeError, match="theta has no element 'mean'"):
        R.call(_shim("cv"), fake, R.theta(th), R.nil)


@pytest.mark.gpu
def test_the_shims_equal_the_python_layer(R):
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    locs, X, th, z = _problem(9)
    n, m, nf = 65, 10, 20
    order = np.random.default_rng(11).permutation(z.size)[:n]             # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    nn = host.vecchia_neighbours(locs, m)
    rng = np.random.default_rng(12)
    W, E = np.asfortranarray(rng.standard_normal((n, 3))), np.asfortranarray(rng.standard_normal((n - nf, 3)))
    fold = (np.arange(n) % 7).astype(np.int32)
    group = R.value(R.call("_cocons_hip_vecchia_group", R.real(nn.astype(float)), R.integer([17])))[0]
    wide = np.asarray(R.value(R.call("_cocons_hip_vecchia_group_table", R.real(nn.astype(float)), R.integer(group)))).reshape((n, -1), order="F")
    h = R.call("_cocons_hip_vecchia_create", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)), R.integer([0]),
               R.real(wide.astype(float)))
    f = ca.CoconsVecchiaFit.from_groups(locs, X, z, wl.SMOOTH_LIMITS, nn, max_rows=17)
    try:
        with pytest.raises(RuntimeError, match="cocons_vecchia_unwhiten_grouped: the handle has no plan"):
            R.call(_shim("unwhiten"), h, R.theta(th), R.real(W))
        with pytest.raises(RuntimeError, match="cocons_cv_vecchia_grouped: the handle has no plan"):
            R.call(_shim("cv"), h, R.theta(th, drop_mean=False), R.nil)
        R.call("_cocons_hip_vecchia_set_groups", h, R.integer(group))
        st, x = R.value(R.call(_shim("unwhiten"), h, R.theta(th), R.real(W)))
        assert int(st[0]) == 0 and np.array_equal(x, f.unwhiten_grouped_core(th, W)) and np.array_equal(x, f.unwhiten_core(th, W))
        st, y = R.value(R.call(_shim("sim"), h, R.theta(th, drop_mean=False), R.integer([0]), R.integer([1]), R.real(W)))
        assert int(st[0]) == 0 and np.array_equal(y, f.sim_grouped_core(th, W)) and np.array_equal(y, f.sim_core(th, W))
        st, c = R.value(R.call(_shim("sim"), h, R.theta(th, drop_mean=False), R.integer([nf]), R.integer([1]), R.real(E)))
        assert int(st[0]) == 0 and c.shape == (n - nf, 3)
        assert np.array_equal(c, f.sim_grouped_core(th, E, n_fixed=nf)) and np.array_equal(c, f.sim_core(th, E, n_fixed=nf))
        st, (ut, qd) = R.value(R.call(_shim("whiten_t"), h, R.theta(th), R.real(W)))
        want = f.whiten_t_grouped_core(th, W)
        assert int(st[0]) == 0 and np.array_equal(ut, want[0]) and np.array_equal(np.ravel(qd), want[1])
        assert all(np.array_equal(a, b) for a, b in zip(want, f.whiten_t_core(th, W)))
        for lab in (None, fold):
            st, (resid, var, stats) = R.value(R.call(_shim("cv"), h, R.theta(th, drop_mean=False), R.nil if lab is None else R.integer(lab)))
            wr, wv, ws = f.cv_core(th, lab, stats=True, grouped=True)
            assert int(st[0]) == 0 and np.array_equal(np.asarray(resid).reshape(wr.shape), wr) and np.array_equal(np.ravel(var), wv)
            assert [int(v) for v in stats[:3]] == [ws["singles"], ws["folds"], ws["entries"]]
            plain = f.cv_core(th, lab)
            assert np.array_equal(wr, plain[0]) and np.array_equal(wv, plain[1])
        print("vecchia-group-coef-report glue | unwhiten, sim, conditional sim, whiten_t, leave-one-out and folds through the R "
              "shims | n%d m%d cap17 | bits" % (n, m))
        with pytest.raises(RuntimeError, match="cocons_sim_vecchia_grouped: z_col = 1 is outside 0 .. 0"):
            R.call(_shim("sim"), h, R.theta(th, drop_mean=False), R.integer([0]), R.integer([2]), R.real(W))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
