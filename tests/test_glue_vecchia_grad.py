"""The Vecchia gradient's shim of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in (tests/test_glue_exec.py's RStub),
like tests/test_glue_vecchia.py: `_cocons_hip_vecchia_neg2loglik_grad` is registered with its arity, the R wrapper calls it,
INTEGRATION.md names both, and on the GPU it returns what tests/vecchia_grad_reference.py computes (bound: 1e-7 of the largest
magnitude of the reference array, the gradients' bound of test_gpu_vecchia_grad.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_grad_reference as VG  # noqa: E402
from test_glue_exec import RStub, _problem  # noqa: E402
from test_glue_vecchia import _handle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 1e-7


@pytest.fixture(scope="module")
def R():
    return RStub()


def test_registration_wrapper_and_documents(R):
    assert R.L.stub_registered_arity(b"_cocons_hip_vecchia_neg2loglik_grad") == 3
    rfile = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    body = rfile[rfile.index(".cocons.hip.vecchia.neg2loglik.grad <- function"):]
    assert "`_cocons_hip_vecchia_neg2loglik_grad`" in body[:body.index("\n}\n")]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_neg2loglik_grad_vecchia", ".cocons.hip.vecchia.neg2loglik.grad"):
        assert entry in doc


@pytest.mark.gpu
def test_value_and_gradient_through_the_glue(R):
    from cocons_amd import host, workloads as wl
    locs, X, th, z = _problem(14)
    order = np.random.default_rng(11).permutation(z.size)
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    nn = host.vecchia_neighbours(locs, 12)
    want = VG.neg2loglik_grad(host.theta_table(th), th["mean"], locs, X, z, wl.SMOOTH_LIMITS, nn)
    h = _handle(R, locs, X, z, nn)
    st, v = R.value(R.call("_cocons_hip_vecchia_neg2loglik", h, R.theta(th), R.real(th["mean"])))
    st, res = R.value(R.call("_cocons_hip_vecchia_neg2loglik_grad", h, R.theta(th), R.real(th["mean"])))
    val, gt, gq, gm = res
    assert int(st[0]) == 0 and gt.shape == (6, 3) and gq.shape == (6, 3) and gm.shape == (3,)
    assert float(np.ravel(val)[0]) == v[0]                       # the value entry's bits
    scale = np.max(np.abs(want[2]))
    errs = [float(np.max(np.abs(gt - want[2])) / scale), float(np.max(np.abs(gq - want[3])) / scale),
            float(np.max(np.abs(gm - want[4])) / np.max(np.abs(want[4])))]
    print("vecchia-grad-report glue | table quad mean | n%d m12 | %.2e" % (z.size, max(errs)))
    assert max(errs) < GRAD_TOL, errs
    # a failing block is a status with zero gradients, not an R error
    nan = {k: np.array(a, dtype=float) for k, a in th.items()}
    nan["scale"][1] = np.nan
    st, res = R.value(R.call("_cocons_hip_vecchia_neg2loglik_grad", h, R.theta(nan), R.real(th["mean"])))
    assert int(st[0]) > 0 and np.all(res[1] == 0.0) and np.all(res[3] == 0.0)
    with pytest.raises(RuntimeError, match="theta\\$mean must have length 3"):
        R.call("_cocons_hip_vecchia_neg2loglik_grad", h, R.theta(th), R.real([0.0]))
    R.call("_cocons_hip_fit_close", h)
