"""The Vecchia neighbour search at the boundary, without a GPU: the headers declare cocons_vecchia_neighbours,
cocons_fit_create_vecchia_knn, cocons_vecchia_predict_knn and cocons_debug_knn_plan, the library exports them and the ctypes
binding carries them; every bad call is refused with -1 (NULL) and a message naming the entry before any HIP call (a HIP call
without a device fails with another code and another message), with the outputs untouched; the R glue registers its three
entries, the R wrappers call them, INTEGRATION.md names them, and the host layer exports the new functions and methods."""
import ctypes
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_vecchia_neighbours": (r"int\s+cocons_vecchia_neighbours\s*\(\s*int n,\s*const double \*locs,\s*int mq,\s*"
                                  r"const double \*locs_query[^,]*,\s*int m,\s*int device,\s*int \*nn[^)]*\)\s*;", 7),
    "cocons_fit_create_vecchia_knn": (r"cocons_fit\s*\*\s*cocons_fit_create_vecchia_knn\s*\(\s*int n,\s*int p,\s*int r,\s*"
                                      r"const double \*locs,\s*const double \*X,\s*const double \*z,\s*"
                                      r"const double \*smooth_limits,\s*int device,\s*int m\s*\)\s*;", 9),
    "cocons_vecchia_predict_knn": (r"int\s+cocons_vecchia_predict_knn\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*"
                                   r"const double \*mean,\s*int z_col,\s*int mp,\s*const double \*locs_pred,\s*"
                                   r"const double \*X_pred,\s*int m_pred,\s*double \*stochastic,\s*double \*quadform\s*\)\s*;", 10),
}


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_headers_declare_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    for name, (pat, nargs) in DECLS.items():
        assert re.search(pat, h), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name)
    d = open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read()
    assert re.search(r"int\s+cocons_debug_knn_plan\s*\(\s*int n,\s*const double \*locs,\s*int level,\s*int m,\s*"
                     r"const double \*pts,\s*int rmax,\s*int \*plan,\s*double \*geom5,\s*int \*cells,\s*double \*bounds\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_knn_plan"][1]) == 10 and hasattr(L, "cocons_debug_knn_plan")
    assert re.search(r"int\s+cocons_debug_knn_phases\s*\(\s*int n,\s*const double \*locs,\s*int m,\s*int device,\s*"
                     r"double \*ms2\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_knn_phases"][1]) == 5 and hasattr(L, "cocons_debug_knn_phases")
    assert L.cocons_abi_version() == 1


def test_neighbours_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    name = "cocons_vecchia_neighbours"
    n, mq, m = 4, 3, 2
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    q = np.array([0.1, 0.2, 0.3, 0.0, 0.0, 0.0])
    bad_locs = locs.copy(); bad_locs[5] = np.nan
    inf_locs = locs.copy(); inf_locs[2] = np.inf
    bad_q = q.copy(); bad_q[4] = -np.inf
    nn = np.full(n * 64, -7, dtype=np.int32)

    def call(n_=n, locs_=locs, mq_=0, q_=None, m_=m, nn_=nn):
        return L.cocons_vecchia_neighbours(n_, _dp(locs_), mq_, _dp(q_), m_, 0, _ip(nn_))

    cases = (dict(locs_=None), dict(nn_=None), dict(n_=0), dict(n_=-3), dict(q_=q, mq_=-1), dict(m_=0), dict(m_=64),
             dict(m_=-1), dict(locs_=bad_locs), dict(locs_=inf_locs), dict(q_=bad_q, mq_=mq), dict(q_=q, mq_=mq, m_=64),
             dict(q_=q, mq_=mq, locs_=bad_locs))
    for kw in cases:
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith(name + ":"), (kw, _lib.last_error())
    assert np.all(nn == -7)
    # the timing entry of the diagnostics refuses the same arguments under its own name, before any HIP call
    ms = np.full(2, -7.0)
    for a in ((0, locs, m, ms), (n, None, m, ms), (n, bad_locs, m, ms), (n, locs, 0, ms), (n, locs, 64, ms), (n, locs, m, None)):
        assert L.cocons_debug_knn_phases(a[0], _dp(a[1]), a[2], 0, _dp(a[3])) == -1, a
        assert _lib.last_error().startswith("cocons_debug_knn_phases:"), _lib.last_error()
    assert np.all(ms == -7.0)
    # an empty query set is no error and no work
    assert call(q_=q, mq_=0) == 0 and np.all(nn == -7)


def test_create_and_predict_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    n, p, mp = 4, 2, 3
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    bad = locs.copy(); bad[1] = np.nan
    X, z, sl = np.ones(n * p), np.ones(n), np.array([0.5, 2.5])

    def create(n_=n, locs_=locs, X_=X, z_=z, sl_=sl, m=2, p_=p, r=1):
        return L.cocons_fit_create_vecchia_knn(n_, p_, r, _dp(locs_), _dp(X_), _dp(z_), _dp(sl_), 0, m)

    for kw in (dict(locs_=None), dict(X_=None), dict(z_=None), dict(sl_=None), dict(n_=0), dict(m=0), dict(m=64), dict(m=-2),
               dict(p_=0), dict(r=0), dict(locs_=bad)):
        assert not create(**kw), kw
        assert _lib.last_error().startswith("cocons_fit_create_vecchia_knn:"), (kw, _lib.last_error())

    name = "cocons_vecchia_predict_knn"
    theta, mean = np.zeros(6 * p), np.zeros(p)
    lp, Xp = np.zeros(mp * 2), np.zeros(mp * p)
    bad_lp = lp.copy(); bad_lp[3] = np.inf
    st, qf = np.full(mp, 7.0), np.full(mp, 7.0)
    fake = ctypes.c_void_p(1)          # never dereferenced: every case below is refused on its arguments alone

    def predict(f=fake, theta_=theta, mean_=mean, mp_=mp, lp_=lp, Xp_=Xp, m_pred=2, st_=st, qf_=qf):
        return L.cocons_vecchia_predict_knn(f, _dp(theta_), _dp(mean_), 0, mp_, _dp(lp_), _dp(Xp_), m_pred, _dp(st_), _dp(qf_))

    assert predict(f=None) == -1
    assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
    for kw in (dict(theta_=None), dict(mean_=None), dict(mp_=-1), dict(lp_=None), dict(Xp_=None), dict(st_=None), dict(qf_=None),
               dict(m_pred=0), dict(m_pred=64), dict(lp_=bad_lp)):
        assert predict(**kw) == -1, kw
        msg = _lib.last_error()
        assert msg.startswith(name + ":") and "null fit handle" not in msg, (kw, msg)
    assert np.all(st == 7.0) and np.all(qf == 7.0)


def test_glue_registers_the_entries_and_r_wrappers_call_them():
    from test_glue_exec import RStub
    R = RStub()
    for name, arity in (("_cocons_hip_vecchia_neighbours", 4), ("_cocons_hip_vecchia_create_knn", 6),
                        ("_cocons_hip_vecchia_predict_knn", 6)):
        assert R.L.stub_registered_arity(name.encode()) == arity, name
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry in ((r"\.cocons\.hip\.vecchia\.neighbours", "_cocons_hip_vecchia_neighbours"),
                      (r"\.cocons\.hip\.vecchia\.create\.knn", "_cocons_hip_vecchia_create_knn"),
                      (r"\.cocons\.hip\.vecchia\.predict\.knn", "_cocons_hip_vecchia_predict_knn")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_vecchia_neighbours", "cocons_fit_create_vecchia_knn", "cocons_vecchia_predict_knn",
                  "_cocons_hip_vecchia_neighbours", "_cocons_hip_vecchia_create_knn", "_cocons_hip_vecchia_predict_knn",
                  ".cocons.hip.vecchia.neighbours", ".cocons.hip.vecchia.create.knn", ".cocons.hip.vecchia.predict.knn"):
        assert entry in doc, entry


def test_host_layer_exports_the_functions_and_the_methods():
    import cocons_amd as ca
    for name in ("vecchia_neighbours_device", "vecchia_neighbours_pred_device", "cocoPredict_vecchia_knn"):
        assert callable(getattr(ca, name)), name
    for name in ("from_knn", "predict_knn_core"):
        assert callable(getattr(ca.CoconsVecchiaFit, name)), name
    assert list(inspect.signature(ca.vecchia_neighbours_device).parameters)[:2] == ["locs", "m"]
    assert list(inspect.signature(ca.vecchia_neighbours_pred_device).parameters)[:3] == ["locs", "newlocs", "m"]
    sig = inspect.signature(ca.CoconsVecchiaFit.from_knn)
    assert list(sig.parameters) == ["locs", "x_covariates", "z", "smooth_limits", "m", "device"] and sig.parameters["device"].default == -1
    sig = inspect.signature(ca.CoconsVecchiaFit.predict_knn_core)
    assert list(sig.parameters)[1:] == ["theta_list", "locs_pred", "x_covariates_pred", "m_pred", "z_col"]
    assert "nn_pred" not in inspect.signature(ca.cocoPredict_vecchia_knn).parameters
    # the existing functions keep their signatures
    assert list(inspect.signature(ca.vecchia_neighbours).parameters) == ["locs", "m"]
    assert list(inspect.signature(ca.cocoPredict_vecchia).parameters)[7] == "nn_pred"
