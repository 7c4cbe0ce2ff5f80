"""The Vecchia information's shim of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in (tests/test_glue_exec.py's
RStub), like tests/test_glue_vecchia_grad.py: `_cocons_hip_vecchia_fisher` returns the bits of the Python entry on the same
data, which tests/test_gpu_vecchia_fisher.py holds to the numpy statement; a failing block is a status, a dirs matrix of the
wrong shape an R error."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
import vecchia_fisher_reference as VF  # noqa: E402
from test_glue_exec import RStub, _problem  # noqa: E402
from test_glue_vecchia import _handle  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-7


@pytest.fixture(scope="module")
def R():
    return RStub()


def test_the_information_through_the_glue(R):
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    nn = host.vecchia_neighbours(locs, 12)
    D = np.concatenate([np.eye(18).reshape(18, 6, 3), FR.scaling_direction(3)[None]])
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        want = f.fisher_core(th, D)
    finally:
        f.close()
    h = _handle(R, locs, X, z, nn)
    dirs = np.asfortranarray(D.reshape(19, 18).T)                 # one direction per column
    st, res = R.value(R.call("_cocons_hip_vecchia_fisher", h, R.theta(th), R.real(dirs)))
    info, im = res
    assert int(st[0]) == 0 and info.shape == (19, 19) and im.shape == (3, 3)
    assert np.array_equal(info, want[0]) and np.array_equal(im, want[1])       # the Python entry's bits
    ref = VF.statement(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, D, nn, 1)
    gap = FR.metric(info, ref[0])
    print("vecchia-fisher-report glue | info (metric) | n%d m12 ndir19 | %.2e" % (z.size, gap))
    assert gap <= TOL
    # a failing block is a status with zero matrices, not an R error
    nan = {k: np.array(a, dtype=float) for k, a in th.items()}
    nan["scale"][1] = np.nan
    st, res = R.value(R.call("_cocons_hip_vecchia_fisher", h, R.theta(nan), R.real(dirs)))
    assert int(st[0]) > 0 and np.all(res[0] == 0.0) and np.all(res[1] == 0.0)
    with pytest.raises(RuntimeError, match="dirs must be a double matrix with 18 rows"):
        R.call("_cocons_hip_vecchia_fisher", h, R.theta(th), R.real(np.zeros((17, 2))))
    R.call("_cocons_hip_fit_close", h)
