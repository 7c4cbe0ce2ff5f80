"""The host wrappers' own contract, for every one of them: what cocons_amd/host.py adds around the library's cores.

1. A borrowed handle (`fit=`) and a handle the wrapper makes and closes itself give the same bits.
2. The safe-objective contract of R/neg2loglikelihood.R:200-206 in all 17 objective wrappers: a failing Cholesky gives exactly
   1e6 under `safe` ((1e6, zeros of theta's shape) in the value + gradient forms), RuntimeError("Cholesky error") otherwise, and
   the handle gives the good theta's bits afterwards.  The failing theta is the optimiser's vector with a NaN in its first
   covariance parameter (tv_nan of test_gpu_taper_sizes.test_failure_and_recovery); it fails in every family.
3. The tail of cocoPredict (R/predict.R:165-177) behind all five prediction wrappers, restated here from the core's
   (stochastic, quadform), to the bit, for type = "mean" and type = "pred".

Nothing here measures a kernel, so one small real problem serves: n = 156 on a 13 x 12 grid, p = 3, two realisations, 20 new
locations, a wend1 taper at delta = 0.15, ten Vecchia neighbours.  Every comparison is for equality."""
import functools
from collections import OrderedDict, namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAM = (0.05, 0.02, 0.3)
DELTA = 0.15
Problem = namedtuple("Problem", "locs X z theta newlocs Xp ref_taper pred_taper nn nn_pred")


@functools.lru_cache(maxsize=None)
def problem():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(156)
    locs = wl.grid_locs(13, 12)
    sc = wl.design_from_locs(locs)
    X = sc["std.covs"]
    newlocs = rng.uniform(0.05, 0.95, size=(20, 2))
    Xp = wl.design_from_locs(newlocs, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    z = rng.standard_normal((156, 2))
    theta = wl.theta_full(scale0=np.log(0.2))
    theta["mean"] = np.array([0.3, -0.1, 0.2])
    out = Problem(locs, X, z, theta, newlocs, Xp, ca.taper_pattern(locs, DELTA, "wend1"),
                  ca.taper_pattern(locs, DELTA, "wend1", newlocs=newlocs), ca.vecchia_neighbours(locs, 10),
                  ca.vecchia_neighbours_pred(locs, newlocs, 10))
    for a in (locs, X, z, newlocs, Xp, out.nn, out.nn_pred) + tuple(out.ref_taper) + tuple(out.pred_taper) + tuple(theta.values()):
        a.setflags(write=False)
    return out


def _vectors(free_mean):
    """(par_pos, the good vector, the same with a NaN in its first covariance parameter)"""
    from cocons_amd import workloads as wl
    p = problem()
    pp = wl.par_pos_full()
    th = OrderedDict((k, np.array(v)) for k, v in p.theta.items())
    first = 0
    if free_mean:
        pp["mean"] = [True] * 3
        first = 3
    else:
        th["mean"] = np.zeros(3)
    tv = wl.theta_vector_from_lists(th, pp)
    tv_nan = tv.copy()
    tv_nan[first] = np.nan
    return pp, tv, tv_nan


def _handle(kind):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    p = problem()
    if kind == "dense":
        return ca.CoconsFit(p.locs, p.X, p.z, wl.SMOOTH_LIMITS)
    if kind == "dense_betas":
        return ca.CoconsFit(p.locs, p.X, p.z, wl.SMOOTH_LIMITS, x_betas=p.X)
    if kind == "taper":
        return ca.CoconsTaperFit(p.locs, p.X, p.z, wl.SMOOTH_LIMITS, *p.ref_taper)
    return ca.CoconsVecchiaFit(p.locs, p.X, p.z, wl.SMOOTH_LIMITS, p.nn)


def _dense(p, sl):
    return (), (p.locs, p.X, sl, p.z, 156, LAM)


def _dense_profile(p, sl):
    return (), (p.locs, p.X, sl, p.z, 156, p.X, LAM)


def _dense_reml(p, sl):
    return (), (p.locs, p.X, p.X, sl, p.z, 156, LAM)


def _taper(p, sl):
    return (p.ref_taper,), (p.locs, p.X, sl, p.z, 156, LAM)


def _vecchia(p, sl):
    return (p.nn,), (p.locs, p.X, sl, p.z, 156, LAM)


def _vecchia_profile(p, sl):
    return (p.nn,), (p.locs, p.X, sl, p.z, 156, p.X, LAM)


def _vecchia_reml(p, sl):
    return (p.nn,), (p.locs, p.X, p.X, sl, p.z, 156, LAM)


# (wrapper, the arguments behind (theta, par_pos), the matching handle, the mean is free, it returns (value, gradient))
WRAPPERS = (
    ("GetNeg2loglikelihood", _dense, "dense", True, False),
    ("GetNeg2loglikelihood_grad", _dense, "dense", True, True),
    ("GetNeg2loglikelihoodProfile", _dense_profile, "dense_betas", False, False),
    ("GetNeg2loglikelihoodREML", _dense_reml, "dense", False, False),
    ("GetNeg2loglikelihoodProfile_grad", _dense_profile, "dense_betas", False, True),
    ("GetNeg2loglikelihoodREML_grad", _dense_reml, "dense", False, True),
    ("GetNeg2loglikelihoodTaper", _taper, "taper", True, False),
    ("GetNeg2loglikelihoodTaperProfile", _taper, "taper", True, False),
    ("GetNeg2loglikelihoodTaper_grad", _taper, "taper", True, True),
    ("GetNeg2loglikelihoodTaperProfile_grad", _taper, "taper", True, True),
    ("GetNeg2loglikelihoodVecchia", _vecchia, "vecchia", True, False),
    ("GetNeg2loglikelihoodVecchiaProfile", _vecchia_profile, "vecchia", False, False),
    ("GetNeg2loglikelihoodVecchiaREML", _vecchia_reml, "vecchia", False, False),
    ("GetNeg2loglikelihoodVecchia_grad", _vecchia, "vecchia", True, True),
    ("GetNeg2loglikelihoodVecchiaProfile_grad", _vecchia_profile, "vecchia", False, True),
    ("GetNeg2loglikelihoodVecchiaREML_grad", _vecchia_reml, "vecchia", False, True),
)


def _same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and np.array_equal(a, b)


@pytest.mark.parametrize("name,args,kind,free_mean,grad", WRAPPERS, ids=[w[0] for w in WRAPPERS])
def test_objective_wrapper(name, args, kind, free_mean, grad):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    fn = getattr(ca, name)
    pp, tv, tv_nan = _vectors(free_mean)
    head, tail = args(problem(), wl.SMOOTH_LIMITS)

    def call(theta, **kw):
        return fn(theta, pp, *head, *tail, **kw)

    owned = call(tv)
    f = _handle(kind)
    try:
        borrowed = call(tv, fit=f)
        failed = call(tv_nan, fit=f)
        with pytest.raises(RuntimeError, match="Cholesky error") as e:
            call(tv_nan, safe=False, fit=f)
        after = call(tv, fit=f)
    finally:
        f.close()
    failed_owned = call(tv_nan)
    with pytest.raises(RuntimeError, match="Cholesky error") as e_owned:
        call(tv_nan, safe=False)

    if grad:
        assert isinstance(owned, tuple) and len(owned) == 2 and owned[1].shape == tv.shape
        assert np.isfinite(owned[0]) and np.all(np.isfinite(owned[1])) and owned[0] != 1e6
    else:
        assert np.isfinite(owned) and owned != 1e6
    assert _same(borrowed, owned), "a borrowed handle and an owned one differ"
    for got in (failed, failed_owned):
        if grad:
            assert isinstance(got, tuple) and len(got) == 2
            assert got[0] == 1e6 and isinstance(got[0], float)
            assert got[1].shape == tv.shape and got[1].dtype == np.float64 and not got[1].any()
        else:
            assert got == 1e6 and isinstance(got, float)
    assert type(e.value) is RuntimeError and str(e.value) == "Cholesky error"
    assert type(e_owned.value) is RuntimeError and str(e_owned.value) == "Cholesky error"
    assert _same(after, owned), "the handle does not give the good theta's bits after the failures"


def test_batch_wrapper():
    """GetNeg2loglikelihood_batch: the failing point gives 1e6 in place, the others what they give without it."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    p = problem()
    pp, tv, tv_nan = _vectors(True)
    tv2 = tv.copy()
    tv2[4] += 0.01
    tail = (p.locs, p.X, wl.SMOOTH_LIMITS, p.z, 156, LAM)
    owned = ca.GetNeg2loglikelihood_batch([tv, tv2], pp, *tail)
    f = _handle("dense")
    try:
        borrowed = ca.GetNeg2loglikelihood_batch([tv, tv2], pp, *tail, fit=f)
        failed = ca.GetNeg2loglikelihood_batch([tv, tv_nan, tv2], pp, *tail, fit=f)
        with pytest.raises(RuntimeError, match="Cholesky error") as e:
            ca.GetNeg2loglikelihood_batch([tv, tv_nan, tv2], pp, *tail, safe=False, fit=f)
        after = ca.GetNeg2loglikelihood_batch([tv, tv2], pp, *tail, fit=f)
    finally:
        f.close()
    failed_owned = ca.GetNeg2loglikelihood_batch([tv, tv_nan, tv2], pp, *tail)
    assert owned.shape == (2,) and np.all(np.isfinite(owned)) and owned[0] != owned[1] and not np.any(owned == 1e6)
    assert _same(borrowed, owned) and _same(after, owned)
    for got in (failed, failed_owned):
        assert got.shape == (3,) and got.dtype == np.float64
        assert got[1] == 1e6 and got[0] == owned[0] and got[2] == owned[1]
    assert type(e.value) is RuntimeError and str(e.value) == "Cholesky error"


def _tail(theta, Xp, st, qf, type):
    """R/predict.R:165-177"""
    out = {"systematic": Xp @ theta["mean"], "stochastic": st}
    if type == "pred":
        unc = 1 / np.exp(-(Xp @ theta["std.dev"])) + np.exp(Xp @ theta["nugget"])
        unc = unc - qf
        neg = unc < 1e-10
        unc[neg] = np.abs(unc[neg])
        out["sd.pred"] = np.sqrt(unc)
    return out


def _dense_core(f, p):
    return f.predict_core(p.theta, p.newlocs, p.Xp)


def _dense_held_core(f, p):
    f.krige_prepare(p.theta)
    try:
        return f.krige_core(p.newlocs, p.Xp)
    finally:
        f.krige_release()


def _taper_core(f, p):
    return f.predict_core(p.theta, p.newlocs, p.Xp, p.pred_taper)


def _taper_held_core(f, p):
    f.krige_taper_prepare(p.theta)
    try:
        return f.krige_taper_core(p.newlocs, p.Xp, p.pred_taper)
    finally:
        f.krige_taper_release()


def _vecchia_core(f, p):
    return f.predict_core(p.theta, p.newlocs, p.Xp, p.nn_pred)


# (wrapper, handle, the core it stands on, what it takes between z and type)
PREDICTORS = (
    ("cocoPredict_dense", "dense", _dense_core, lambda p: ()),
    ("cocoPredict_dense_chunked", "dense", _dense_held_core, lambda p: ()),
    ("cocoPredict_sparse", "taper", _taper_core, lambda p: (p.ref_taper, p.pred_taper)),
    ("cocoPredict_sparse_chunked", "taper", _taper_held_core, lambda p: (p.ref_taper, p.pred_taper)),
    ("cocoPredict_vecchia", "vecchia", _vecchia_core, lambda p: (p.nn_pred,)),
)


@pytest.mark.parametrize("name,kind,core,extra", PREDICTORS, ids=[w[0] for w in PREDICTORS])
def test_predict_tail(name, kind, core, extra):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    p = problem()
    fn = getattr(ca, name)
    args = (p.theta, p.locs, p.newlocs, p.X, p.Xp, wl.SMOOTH_LIMITS, p.z) + extra(p)
    f = _handle(kind)
    try:
        st, qf = core(f, p)
        borrowed = {t: fn(*args, type=t, fit=f) for t in ("mean", "pred")}
    finally:
        f.close()
    owned = {t: fn(*args, type=t) for t in ("mean", "pred")}
    assert st.shape == qf.shape == (20,) and np.all(np.isfinite(st)) and np.all(qf > 0)
    for t in ("mean", "pred"):
        want = _tail(p.theta, p.Xp, st, qf, t)
        assert list(want) == ["systematic", "stochastic"] + (["sd.pred"] if t == "pred" else [])
        for got in (borrowed[t], owned[t]):
            assert type(got) is dict and list(got) == list(want)
            for k in want:
                assert got[k].shape == (20,) and got[k].dtype == np.float64
                assert np.array_equal(got[k], want[k]), (t, k)
    assert np.all(want["sd.pred"] > 0)
