"""The Vecchia shims of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way tests/test_glue_exec.py drives the
others (its RStub): `_cocons_hip_vecchia_create`, `_cocons_hip_vecchia_neg2loglik`, `_cocons_hip_vecchia_predict` are
registered with their arities, refuse bad tables as R errors before any device work, and on the GPU return what
tests/vecchia_reference.py computes on the oracle's matrices (bound: the project's parity bound 1e-8)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_reference as VR  # noqa: E402
from test_glue_exec import RStub, _problem  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = 1e-8


@pytest.fixture(scope="module")
def R():
    return RStub()


def _handle(R, locs, X, z, nn):
    from cocons_amd import workloads as wl
    return R.call("_cocons_hip_vecchia_create", R.real(locs), R.real(X), R.real(z), R.real(list(wl.SMOOTH_LIMITS)),
                  R.integer([0]), R.real(np.asarray(nn, dtype=float)))


def test_registration_and_refusals_without_a_device(R):
    for name, arity in {"_cocons_hip_vecchia_create": 6, "_cocons_hip_vecchia_neg2loglik": 3,
                        "_cocons_hip_vecchia_predict": 6}.items():
        assert R.L.stub_registered_arity(name.encode()) == arity
    rfile = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for wrapper, sym in ((".cocons.hip.vecchia.create", "_cocons_hip_vecchia_create"),
                         (".cocons.hip.vecchia.neg2loglik", "_cocons_hip_vecchia_neg2loglik"),
                         (".cocons.hip.vecchia.predict", "_cocons_hip_vecchia_predict")):
        body = rfile[rfile.index(wrapper + " <- function"):]
        assert "`%s`" % sym in body[:body.index("\n}\n")]
    locs, X, th, z = _problem(6)
    n = z.size
    z = z.reshape(n, 1)
    with pytest.raises(RuntimeError, match="cocons_fit_create_vecchia: m = 64 is outside 1 .. 63"):
        _handle(R, locs, X, z, np.zeros((n, 64)))
    late = np.zeros((n, 2))
    late[4, 1] = 5                                    # row 5 names itself
    with pytest.raises(RuntimeError, match="cocons_fit_create_vecchia: row 5 of nn names an index outside its range"):
        _handle(R, locs, X, z, late)
    twice = np.zeros((n, 2))
    twice[7] = 3
    with pytest.raises(RuntimeError, match="cocons_fit_create_vecchia: row 8 of nn names an index twice"):
        _handle(R, locs, X, z, twice)
    with pytest.raises(RuntimeError, match="nn must be a matrix with one row per observation"):
        _handle(R, locs, X, z, np.zeros((n - 1, 2)))


@pytest.mark.gpu
def test_value_prediction_and_status_through_the_glue(R, oracle):
    from cocons_amd import host, workloads as wl
    locs, X, th, z = _problem(14)
    rng = np.random.default_rng(11)
    order = rng.permutation(z.size)                   # a random Vecchia order
    locs, X, z = locs[order], np.asfortranarray(X[order]), z[order].reshape(-1, 1)
    n = z.size
    nn = host.vecchia_neighbours(locs, 12)
    S = oracle.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
    Rz = z - (X @ th["mean"])[:, None]
    want, parts = VR.neg2loglik(S, nn, Rz)
    h = _handle(R, locs, X, z, nn)
    st, v = R.value(R.call("_cocons_hip_vecchia_neg2loglik", h, R.theta(th), R.real(th["mean"])))
    assert int(st[0]) == 0 and v.shape == (3,)
    errs = [abs(v[0] - want) / abs(want), float(np.max(np.abs(v[1:] - parts)) / np.max(np.abs(parts)))]
    lp = locs[:21] + 0.013
    lp[5] = locs[9]                                   # on an observation that is among its neighbours
    Xp = np.asfortranarray(X[:21] * 0.9)
    nnp = host.vecchia_neighbours_pred(locs, lp, 9)
    assert 10 in nnp[5]
    C = oracle.cov_rns_pred(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS)
    ws, wq = VR.predict(S, C, nnp, Rz[:, 0])
    st, kr = R.value(R.call("_cocons_hip_vecchia_predict", h, R.theta(th, drop_mean=False), R.integer([1]), R.real(lp),
                            R.real(Xp), R.real(nnp.astype(float))))
    assert int(st[0]) == 0 and kr.shape == (21, 2)
    errs += [float(np.max(np.abs(kr[:, 0] - ws)) / np.max(np.abs(ws))), float(np.max(np.abs(kr[:, 1] - wq)) / np.max(np.abs(wq)))]
    print("vecchia-report glue | value parts stochastic quadform | n%d m12 | %.2e" % (n, max(errs)))
    assert max(errs) < PARITY, errs
    # a failing block is a status, not an R error: list(status = row, NA ...)
    nan = {k: np.array(val, dtype=float) for k, val in th.items()}
    nan["scale"][1] = np.nan
    st, v = R.value(R.call("_cocons_hip_vecchia_neg2loglik", h, R.theta(nan), R.real(th["mean"])))
    assert int(st[0]) > 0 and np.all(np.isnan(v))
    # the dense entry refuses the handle with a message (an R error)
    with pytest.raises(RuntimeError, match="not available on a Vecchia fit"):
        R.call("_cocons_hip_neg2loglik", h, R.theta(th), R.real(th["mean"]))
    with pytest.raises(RuntimeError, match="theta\\$mean must have length 3"):
        R.call("_cocons_hip_vecchia_neg2loglik", h, R.theta(th), R.real([0.0]))
    with pytest.raises(RuntimeError, match="theta has no element 'mean'"):
        R.call("_cocons_hip_vecchia_predict", h, R.theta(th), R.integer([1]), R.real(lp), R.real(Xp), R.real(nnp.astype(float)))
    R.call("_cocons_hip_fit_close", h)
    assert R.L.stub_extptr(h) is None
