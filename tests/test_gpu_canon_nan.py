"""An all-ones NaN in a caller's array is canonicalised before it reaches the device (fit.hpp: canon_nan; api.hip: upload_canon).

That bit pattern is the factorisation mailboxes' "not written yet" word: if it reached a factor block it would be waited on
until the bounded wait ran out (an engine time-out and a repeat).  One small case per one-shot entry: the call returns in
its normal time with the status a NaN gives, and the handle counts no hand-off time-out.
"""
import struct
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_ONES_NAN = struct.unpack("<d", b"\xff" * 8)[0]
N = 1000


def _problem(seed):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(N, 2))
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full(scale0=np.log(0.2))
    fit = ca.CoconsFit(locs, X, rng.standard_normal(N), wl.SMOOTH_LIMITS)
    return fit, th, rng


def _timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, time.perf_counter() - t0


def _no_timeouts(fit):
    assert fit.engine_state()["retries"] == 0


def _in_normal_time(elapsed, clean):
    assert elapsed < 5 * clean + 0.5, (elapsed, clean)


def test_all_ones_nan_in_predict_mean():
    from cocons_amd import workloads as wl
    fit, th, rng = _problem(61)
    m = 50
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = wl.design_from_locs(lp)["std.covs"]
    fit.predict_core(th, lp, Xp)                                # warm-up
    (st0, qf0), clean = _timed(lambda: fit.predict_core(th, lp, Xp))
    bad = dict(th, mean=np.array(th["mean"], dtype=np.float64))
    bad["mean"][0] = ALL_ONES_NAN
    (st, qf), elapsed = _timed(lambda: fit.predict_core(bad, lp, Xp))
    assert np.isnan(st).all() and np.isfinite(st0).all()       # the residual row carries the NaN ...
    assert np.allclose(qf, qf0, rtol=1e-12, atol=0)            # ... the cross-covariance rows do not depend on the mean
    _in_normal_time(elapsed, clean)
    _no_timeouts(fit)


def test_all_ones_nan_in_sim_iiderrors():
    fit, th, rng = _problem(62)
    E = rng.standard_normal((N, 4))
    fit.sim_core(th, E)                                         # warm-up
    out0, clean = _timed(lambda: fit.sim_core(th, E))
    i = N // 2
    Ebad = E.copy()
    Ebad[i, 1] = ALL_ONES_NAN
    out, elapsed = _timed(lambda: fit.sim_core(th, Ebad))
    assert np.isfinite(out0).all()
    assert np.allclose(out[:, [0, 2, 3]], out0[:, [0, 2, 3]], rtol=1e-12, atol=1e-14)   # the other draws are untouched
    assert np.isnan(out[:, 1]).any()
    _in_normal_time(elapsed, clean)
    _no_timeouts(fit)


def test_all_ones_nan_in_sim_cond_x_pred():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    fit, th, rng = _problem(63)
    m = 40
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = np.array(wl.design_from_locs(lp)["std.covs"], dtype=np.float64)
    E = rng.standard_normal((m, 3))
    fit.sim_cond_core(th, lp, Xp, lp, E)                        # warm-up
    out0, clean = _timed(lambda: fit.sim_cond_core(th, lp, Xp, lp, E))
    assert np.isfinite(out0).all()
    Xbad = Xp.copy()
    Xbad[m // 2, 1] = ALL_ONES_NAN                              # a NaN in the Schur block: its pivot is not positive
    t0 = time.perf_counter()
    with pytest.raises(ca.CholeskyError):
        fit.sim_cond_core(th, lp, Xbad, lp, E)
    _in_normal_time(time.perf_counter() - t0, clean)
    _no_timeouts(fit)
