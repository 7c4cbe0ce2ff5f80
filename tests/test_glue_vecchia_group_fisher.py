"""The grouped-information shim of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way
tests/test_glue_vecchia_group_grad.py drives the grouped gradient shim: `_cocons_hip_vecchia_fisher_grouped` is registered with
its arity, named by its R wrapper, refuses bad arguments as R errors before any device work, and on the GPU returns what the C
entry returns through the Python core, to the bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
from test_glue_exec import ROOT, RStub, _problem  # noqa: E402

SHIM = "_cocons_hip_vecchia_fisher_grouped"


@pytest.fixture(scope="module")
def R():
    return RStub()


def test_registration_and_refusals_without_a_device(R):
    assert R.L.stub_registered_arity(SHIM.encode()) == 3
    rfile = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    body = rfile[rfile.index(".cocons.hip.vecchia.fisher.grouped <- function"):]
    assert ".cocons.hip.vecchia.fisher(" in body[:body.index("\n}\n")]           # the Jacobian code is the ungrouped wrapper's
    shared = rfile[rfile.index(".cocons.hip.vecchia.fisher <- function"):]
    assert "`%s`" % SHIM in shared[:shared.index("\n}\n")]
    th = _problem(8)[2]
    R.L.R_MakeExternalPtr.restype, R.L.R_MakeExternalPtr.argtypes = ctypes.c_void_p, [ctypes.c_void_p] * 3
    closed = R.L.R_MakeExternalPtr(None, R.nil, R.nil)                      # a handle restored from a saved workspace
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call(SHIM, closed, R.theta(th), R.real(np.zeros((18, 2))))
    fake = R.L.R_MakeExternalPtr(ctypes.c_void_p(1), R.integer([64, 3, 1, 0]), R.nil)     # its address is never used
    with pytest.raises(RuntimeError, match="dirs must be a double matrix with 18 rows"):
        R.call(SHIM, fake, R.theta(th), R.real(np.zeros((17, 2))))


@pytest.mark.gpu
def test_the_wrapper_equals_the_c_entry(R):
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n, m = z.size, 12
    nn = host.vecchia_neighbours(locs, m)
    D = np.concatenate([np.eye(18).reshape(18, 6, 3), FR.scaling_direction(3)[None]])
    dirs = np.asfortranarray(D.reshape(19, 18).T)                         # one direction per column
    group = R.value(R.call("_cocons_hip_vecchia_group", R.real(nn.astype(float)), R.integer([64])))[0]
    wide = np.asarray(R.value(R.call("_cocons_hip_vecchia_group_table", R.real(nn.astype(float)), R.integer(group)))).reshape((n, -1), order="F")
    h = R.call("_cocons_hip_vecchia_create", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)), R.integer([0]),
               R.real(wide.astype(float)))
    f = ca.CoconsVecchiaFit.from_groups(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        with pytest.raises(RuntimeError, match="cocons_fisher_vecchia_grouped: the handle has no plan"):
            R.call(SHIM, h, R.theta(th), R.real(dirs))
        R.call("_cocons_hip_vecchia_set_groups", h, R.integer(group))
        st, res = R.value(R.call(SHIM, h, R.theta(th), R.real(dirs)))
        want = f.fisher_core(th, D, grouped=True)
        assert int(st[0]) == 0 and res[0].shape == (19, 19) and res[1].shape == (3, 3)
        assert np.array_equal(res[0], want[0]) and np.array_equal(res[1], want[1])
        gap = FR.metric(res[0], f.fisher_core(th, D)[0])
        print("vecchia-group-fisher-report glue | info through the R shim against the ungrouped entry (metric) | n%d m%d ndir19 | %.2e"
              % (n, m, gap))
        assert gap <= 1e-7
        # a failing block is a status with zero matrices, not an R error
        nan = {k: np.array(a, dtype=float) for k, a in th.items()}
        nan["scale"][1] = np.nan
        st, res = R.value(R.call(SHIM, h, R.theta(nan), R.real(dirs)))
        assert int(st[0]) > 0 and np.all(res[0] == 0.0) and np.all(res[1] == 0.0)
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
