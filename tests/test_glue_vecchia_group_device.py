"""The round rule's shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in on the GPU, the way
tests/test_glue_vecchia_group.py drives the greedy rule's: `_cocons_hip_vecchia_group_device`,
`_cocons_hip_vecchia_create_grouped_knn` and `_cocons_hip_vecchia_groups_export` return what the Python layer returns, to the
integer and to the bit.  (Registration and the host shim: tests/test_group_rounds_abi.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_glue_exec import ROOT, RStub, _problem  # noqa: E402

pytestmark = pytest.mark.gpu

SHIMS = {"_cocons_hip_vecchia_group_rounds": 3, "_cocons_hip_vecchia_group_device": 4, "_cocons_hip_vecchia_create_grouped_knn": 8,
         "_cocons_hip_vecchia_groups_export": 1}
WRAPPERS = {".cocons.hip.vecchia.group.rounds": "_cocons_hip_vecchia_group_rounds",
            ".cocons.hip.vecchia.group.device": "_cocons_hip_vecchia_group_device",
            ".cocons.hip.vecchia.create.grouped.knn": "_cocons_hip_vecchia_create_grouped_knn",
            ".cocons.hip.vecchia.groups.export": "_cocons_hip_vecchia_groups_export"}


@pytest.fixture(scope="module")
def R():
    return RStub()


def test_the_shims_equal_the_python_results(R):
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    for name, arity in SHIMS.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    rfile = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for wrapper, sym in WRAPPERS.items():
        body = rfile[rfile.index(wrapper + " <- function"):]
        assert "`%s`" % sym in body[:body.index("\n}\n")]
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n, m = z.size, 12
    nn = host.vecchia_neighbours_device(locs, m)
    want, st = host.vecchia_group_rounds(nn, 64, stats=True)
    group, info = R.value(R.call("_cocons_hip_vecchia_group_device", R.real(nn.astype(float)), R.integer([64]), R.integer([0]),
                                 R.integer([0])))
    assert np.array_equal(group, want)
    assert [int(v) for v in info] == [st["blocks"], st["rows"], st["pairs"], st["pairs_ungrouped"], st["rounds"]]
    h = R.call("_cocons_hip_vecchia_create_grouped_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]), R.integer([m]), R.integer([64]), R.integer([0]))
    f = ca.CoconsVecchiaFit.from_groups_knn(locs, X, z, wl.SMOOTH_LIMITS, m)
    try:
        block, tab = R.value(R.call("_cocons_hip_vecchia_groups_export", h))
        fb, ft = f.groups_export()
        assert np.array_equal(block, want) and np.array_equal(fb, want)
        assert np.array_equal(np.asarray(tab).reshape((n, -1), order="F"), ft)
        assert np.array_equal(ft, host.vecchia_group_table(nn, want))
        st_, v = R.value(R.call("_cocons_hip_vecchia_neg2loglik_grouped", h, R.theta(th), R.real(th["mean"])))
        val, parts = f.neg2loglik_core(th, grouped=True)
        assert int(st_[0]) == 0 and v[0] == val and np.array_equal(v[1:], parts)
        print("vecchia-group-device-report glue | group.device, create.grouped.knn, groups.export and the grouped value through the "
              "R shims | n%d m%d | blocks %d | integers and bits" % (n, m, st["blocks"]))
        with pytest.raises(RuntimeError, match="cocons_fit_create_vecchia_grouped_knn: max_rows = 65 is outside 2 .. 64"):
            R.call("_cocons_hip_vecchia_create_grouped_knn", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
                   R.integer([0]), R.integer([m]), R.integer([65]), R.integer([0]))
    finally:
        f.close()
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
