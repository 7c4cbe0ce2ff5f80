"""The grouped-block shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way
tests/test_glue_vecchia_cv.py drives the U' shims: `_cocons_hip_vecchia_group`, `_cocons_hip_vecchia_group_table`,
`_cocons_hip_vecchia_set_groups`, `_cocons_hip_vecchia_neg2loglik_grouped` and `_cocons_hip_vecchia_whiten_grouped` are
registered with their arities, named by their R wrappers, refuse bad arguments as R errors before any device work, and on the
GPU return what the Python layer returns, to the bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
from test_glue_exec import ROOT, RStub, _problem  # noqa: E402

SHIMS = {"_cocons_hip_vecchia_group": 2, "_cocons_hip_vecchia_group_table": 2, "_cocons_hip_vecchia_set_groups": 2,
         "_cocons_hip_vecchia_neg2loglik_grouped": 3, "_cocons_hip_vecchia_whiten_grouped": 3}
WRAPPERS = {".cocons.hip.vecchia.group": "_cocons_hip_vecchia_group", ".cocons.hip.vecchia.group.table": "_cocons_hip_vecchia_group_table",
            ".cocons.hip.vecchia.set.groups": "_cocons_hip_vecchia_set_groups",
            ".cocons.hip.vecchia.neg2loglik.grouped": "_cocons_hip_vecchia_neg2loglik_grouped",
            ".cocons.hip.vecchia.whiten.grouped": "_cocons_hip_vecchia_whiten_grouped"}


@pytest.fixture(scope="module")
def R():
    return RStub()


def _table(locs, m):
    from cocons_amd import host
    return host.vecchia_neighbours(locs, m)


def test_registration_host_entries_and_refusals_without_a_device(R):
    for name, arity in SHIMS.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    rfile = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for wrapper, sym in WRAPPERS.items():
        body = rfile[rfile.index(wrapper + " <- function"):]
        assert "`%s`" % sym in body[:body.index("\n}\n")]
    locs, X, th, z = _problem(8)
    n, m = z.size, 6
    nn = _table(locs, m)
    # the two host entries need no device: the groups and the expanded table of the restatement
    group, info = R.value(R.call("_cocons_hip_vecchia_group", R.real(nn.astype(float)), R.integer([17])))
    want = GR.greedy(nn, 17)
    pl = GR.plan(nn, want)
    assert np.array_equal(group, want)
    assert [int(v) for v in info] == [pl["blocks"], pl["sum_rows"], pl["pairs"], GR.pairs_ungrouped(nn)]
    wide = R.call("_cocons_hip_vecchia_group_table", R.real(nn.astype(float)), R.integer(want))
    assert (R.L.stub_nrow(wide), R.L.stub_ncol(wide)) == (n, max(pl["longest"], 1))
    assert np.array_equal(np.asarray(R.value(wide)).reshape((n, -1), order="F"), GR.table(nn, want))
    with pytest.raises(RuntimeError, match="cocons_vecchia_group: max_rows = 65 is outside 2 .. 64"):
        R.call("_cocons_hip_vecchia_group", R.real(nn.astype(float)), R.integer([65]))
    with pytest.raises(RuntimeError, match="nn must be a matrix"):
        R.call("_cocons_hip_vecchia_group", R.real(np.zeros(n)), R.integer([64]))
    with pytest.raises(RuntimeError, match="group must be %d integer labels" % n):
        R.call("_cocons_hip_vecchia_group_table", R.real(nn.astype(float)), R.integer(want[:-1]))
    with pytest.raises(RuntimeError, match="cocons_vecchia_group_table: the block of row 1 spans more than 64 rows"):
        R.call("_cocons_hip_vecchia_group_table", R.real(_table(_problem(9)[0], 30).astype(float)), R.integer(np.zeros(81)))
    R.L.R_MakeExternalPtr.restype, R.L.R_MakeExternalPtr.argtypes = ctypes.c_void_p, [ctypes.c_void_p] * 3
    closed = R.L.R_MakeExternalPtr(None, R.nil, R.nil)                      # a handle restored from a saved workspace
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_set_groups", closed, R.integer(want))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_neg2loglik_grouped", closed, R.theta(th), R.real(th["mean"]))
    with pytest.raises(RuntimeError, match="handle is NULL"):
        R.call("_cocons_hip_vecchia_whiten_grouped", closed, R.theta(th), R.real(np.zeros((n, 1))))
    # a handle of n = 64, p = 3, r = 1 whose address is never used: every call below is refused by the shim on its arguments
    fake = R.L.R_MakeExternalPtr(ctypes.c_void_p(1), R.integer([n, 3, 1, 0]), R.nil)
    with pytest.raises(RuntimeError, match="group must be %d integer labels" % n):
        R.call("_cocons_hip_vecchia_set_groups", fake, R.real(want.astype(float)))
    with pytest.raises(RuntimeError, match="W must be a double matrix with %d rows" % n):
        R.call("_cocons_hip_vecchia_whiten_grouped", fake, R.theta(th), R.real(np.zeros((n - 1, 2))))
    with pytest.raises(RuntimeError, match="mean must have length 3"):
        R.call("_cocons_hip_vecchia_neg2loglik_grouped", fake, R.theta(th), R.real(np.zeros(2)))


@pytest.mark.gpu
def test_the_wrappers_equal_the_python_results(R):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)                 # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n, m = z.size, 12
    nn = _table(locs, m)
    W = np.random.default_rng(12).standard_normal((n, 5))
    group = R.value(R.call("_cocons_hip_vecchia_group", R.real(nn.astype(float)), R.integer([64])))[0]
    wide = np.asarray(R.value(R.call("_cocons_hip_vecchia_group_table", R.real(nn.astype(float)), R.integer(group)))).reshape((n, -1), order="F")
    h = R.call("_cocons_hip_vecchia_create", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)), R.integer([0]),
               R.real(wide.astype(float)))
    f = ca.CoconsVecchiaFit.from_groups(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        with pytest.raises(RuntimeError, match="cocons_neg2loglik_vecchia_grouped: the handle has no plan"):
            R.call("_cocons_hip_vecchia_neg2loglik_grouped", h, R.theta(th), R.real(th["mean"]))
        info = R.value(R.call("_cocons_hip_vecchia_set_groups", h, R.integer(group)))
        gi = f.groups_info()
        assert [int(v) for v in info] == [gi["blocks"], gi["maxrows"], gi["rows"], gi["pairs"], gi["bytes"]]
        st, v = R.value(R.call("_cocons_hip_vecchia_neg2loglik_grouped", h, R.theta(th), R.real(th["mean"])))
        val, parts = f.neg2loglik_core(th, grouped=True)
        assert int(st[0]) == 0 and v[0] == val and np.array_equal(v[1:], parts) and val == f.neg2loglik_core(th)[0]
        st, (out, logd) = R.value(R.call("_cocons_hip_vecchia_whiten_grouped", h, R.theta(th), R.real(W)))
        wo, wl_ = f.whiten_grouped_core(th, W)
        assert int(st[0]) == 0 and np.array_equal(out, wo) and np.array_equal(np.ravel(logd), wl_)
        print("vecchia-group-report glue | groups, table, set_groups, value and whitening through the R wrappers | n%d m%d | "
              "worst deviation %.1e" % (n, m, float(np.max(np.abs(out - wo)))))
        other = np.array(group)
        other[-1] = other[0]
        with pytest.raises(RuntimeError, match="cocons_vecchia_set_groups: "):
            R.call("_cocons_hip_vecchia_set_groups", h, R.integer(other))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
