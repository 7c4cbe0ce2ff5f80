"""The neighbours of new locations by model correlation and the grouped handle on a correlation table at the
boundary, without a GPU: the header declares cocons_vecchia_neighbours_corr_pred, cocons_vecchia_predict_corr_knn and
cocons_fit_create_vecchia_grouped_corr_knn and states their rule, the library exports them and the ctypes binding carries
them; every bad call is refused with -1 (NULL) and a message naming the entry before any HIP call (a HIP call without a device
fails with another code and another message), with the outputs untouched; the host layer exports the restatement and the
methods, and the documents name the entries.  (The refusals that need a live handle -- another kind of handle, a theta that is
not finite on the two prediction entries -- are in test_gpu_corr_knn_pred.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_vecchia_neighbours_corr_pred": (r"int\s+cocons_vecchia_neighbours_corr_pred\s*\(\s*cocons_fit\s*\*\s*fit,\s*"
                                            r"const double \*theta,\s*int mp,\s*const double \*locs_pred,\s*"
                                            r"const double \*X_pred,\s*int m_cand,\s*int hops,\s*int m,\s*int \*nn_out[^)]*\)\s*;", 9),
    "cocons_vecchia_predict_corr_knn": (r"int\s+cocons_vecchia_predict_corr_knn\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*"
                                        r"const double \*mean,\s*int z_col,\s*int mp,\s*const double \*locs_pred,\s*"
                                        r"const double \*X_pred,\s*int m_cand,\s*int hops,\s*int m_pred,\s*double \*stochastic,\s*"
                                        r"double \*quadform\s*\)\s*;", 12),
    "cocons_fit_create_vecchia_grouped_corr_knn": (r"cocons_fit\s*\*\s*cocons_fit_create_vecchia_grouped_corr_knn\s*\(\s*int n,\s*int p,\s*"
                                                   r"int r,\s*const double \*locs,\s*const double \*X,\s*const double \*z,\s*"
                                                   r"const double \*smooth_limits,\s*int device,\s*const double \*theta,\s*"
                                                   r"int m_cand,\s*int hops,\s*int m,\s*int max_rows,\s*int max_rounds\s*\)\s*;", 14),
}


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_header_declares_and_states_the_rule_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    for name, (pat, nargs) in DECLS.items():
        assert re.search(pat, h), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name)
    for phrase in ("fl(v / fl(sqrt(fl(d_q d_j))))", "UNORDERED on purpose", "depends on no other row of the query set and on no chunking",
                   "n <= m_cand ranks\n * every observation", "placed ON an observation", "120 MB",
                   "correlation-ranked neighbours inside the joint handle of cocoPredict_vecchia_joint"):
        assert phrase in h, phrase
    assert "Out of scope: a fused device chain" not in h
    assert L.cocons_abi_version() == 1          # the entries add to the ABI and change nothing in it


def test_prediction_entries_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    theta, mean = np.zeros(6), np.zeros(1)
    mp = 4
    lp, Xp = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5]), np.ones(mp)
    nan_lp = lp.copy(); nan_lp[5] = np.nan
    inf_lp = lp.copy(); inf_lp[2] = np.inf
    nn = np.full(mp * 64, -7, dtype=np.int32)
    st, qf = np.full(mp, -7.0), np.full(mp, -7.0)
    fake = ctypes.c_void_p(1)          # never dereferenced: every case below is refused on its arguments alone

    def table(f=fake, theta_=theta, mp_=mp, lp_=lp, Xp_=Xp, m_cand=5, hops=2, m=3, nn_=nn):
        return L.cocons_vecchia_neighbours_corr_pred(f, _dp(theta_), mp_, _dp(lp_), _dp(Xp_), m_cand, hops, m, _ip(nn_))

    def predict(f=fake, theta_=theta, mean_=mean, mp_=mp, lp_=lp, Xp_=Xp, m_cand=5, hops=2, m=3, st_=st, qf_=qf):
        return L.cocons_vecchia_predict_corr_knn(f, _dp(theta_), _dp(mean_), 0, mp_, _dp(lp_), _dp(Xp_), m_cand, hops, m,
                                                 _dp(st_), _dp(qf_))

    shapes = (dict(m_cand=0), dict(m_cand=64), dict(m_cand=-1), dict(hops=0), dict(hops=3), dict(m=0), dict(m=64), dict(m=-5),
              dict(m_cand=5, hops=1, m=6),             # one hop: at most m_cand candidates
              dict(m_cand=1, hops=2, m=3),             # two hops: at most m_cand + m_cand^2
              dict(m_cand=7, hops=2, m=57))
    common = (dict(theta_=None), dict(lp_=None), dict(Xp_=None), dict(mp_=-1), dict(lp_=nan_lp), dict(lp_=inf_lp))
    for name, call, own in (("cocons_vecchia_neighbours_corr_pred", table, (dict(nn_=None),)),
                            ("cocons_vecchia_predict_corr_knn", predict, (dict(mean_=None), dict(st_=None), dict(qf_=None)))):
        assert call(f=None) == -1
        assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
        for kw in common + own + shapes:
            assert call(**kw) == -1, (name, kw)
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and "null fit handle" not in msg, (kw, msg)
    assert np.all(nn == -7) and np.all(st == -7.0) and np.all(qf == -7.0)


def test_create_grouped_corr_knn_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    name = "cocons_fit_create_vecchia_grouped_corr_knn"
    n, p = 4, 2
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    bad = locs.copy(); bad[1] = np.nan
    X, z, sl, theta = np.ones(n * p), np.ones(n), np.array([0.5, 2.5]), np.zeros(6 * p)
    nan_theta = theta.copy(); nan_theta[7] = np.nan
    inf_theta = theta.copy(); inf_theta[0] = -np.inf

    def create(n_=n, locs_=locs, X_=X, z_=z, sl_=sl, theta_=theta, m_cand=3, hops=2, m=2, p_=p, r=1, max_rows=64, max_rounds=0):
        return L.cocons_fit_create_vecchia_grouped_corr_knn(n_, p_, r, _dp(locs_), _dp(X_), _dp(z_), _dp(sl_), 0, _dp(theta_),
                                                            m_cand, hops, m, max_rows, max_rounds)

    for kw in (dict(locs_=None), dict(X_=None), dict(z_=None), dict(sl_=None), dict(theta_=None), dict(n_=0), dict(p_=0), dict(r=0),
               dict(locs_=bad), dict(theta_=nan_theta), dict(theta_=inf_theta), dict(m_cand=0), dict(m_cand=64), dict(hops=0),
               dict(hops=3), dict(m=0), dict(m=64), dict(m_cand=3, hops=1, m=4), dict(m_cand=2, hops=2, m=7),
               dict(max_rows=1), dict(max_rows=65), dict(max_rounds=-1)):
        assert not create(**kw), kw
        assert _lib.last_error().startswith(name + ":"), (kw, _lib.last_error())


def test_host_layer_exports_the_restatement_and_the_methods():
    import cocons_amd as ca
    assert list(inspect.signature(ca.vecchia_neighbours_corr_pred).parameters) == ["Cq", "dq", "d", "nn_pred", "nn_all", "m", "hops"]
    assert inspect.signature(ca.vecchia_neighbours_corr_pred).parameters["hops"].default == 2
    sig = inspect.signature(ca.CoconsVecchiaFit.neighbours_corr_pred)
    assert list(sig.parameters)[1:] == ["theta_list", "locs_pred", "x_covariates_pred", "m", "m_cand", "hops"]
    assert sig.parameters["m_cand"].default is None and sig.parameters["hops"].default == 2
    sig = inspect.signature(ca.CoconsVecchiaFit.predict_corr_knn_core)
    assert list(sig.parameters)[1:] == ["theta_list", "locs_pred", "x_covariates_pred", "m_pred", "m_cand", "hops", "z_col"]
    for name in ("from_groups_corr_knn", "from_maxmin_groups_corr"):
        sig = inspect.signature(getattr(ca.CoconsVecchiaFit, name))
        assert list(sig.parameters) == ["locs", "x_covariates", "z", "smooth_limits", "theta_list", "m", "m_cand", "hops",
                                        "max_rows", "max_rounds", "device"]
    sig = inspect.signature(ca.cocoPredict_vecchia_corr_knn)
    assert list(sig.parameters) == ["theta_list", "locs", "newlocs", "X_std", "X_pred_std", "smooth_limits", "z", "m_pred", "m_cand",
                                    "hops", "type", "fit"]
    # the existing entries keep their signatures
    assert list(inspect.signature(ca.CoconsVecchiaFit.predict_knn_core).parameters)[1:] == ["theta_list", "locs_pred", "x_covariates_pred",
                                                                                            "m_pred", "z_col"]
    assert list(inspect.signature(ca.CoconsVecchiaFit.from_groups_knn).parameters) == ["locs", "x_covariates", "z", "smooth_limits", "m",
                                                                                       "max_rows", "max_rounds", "device"]


def test_the_documents_name_the_entries():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_vecchia_neighbours_corr_pred", "cocons_vecchia_predict_corr_knn", "cocons_fit_create_vecchia_grouped_corr_knn",
                  "_cocons_hip_vecchia_neighbours_corr_pred", "_cocons_hip_vecchia_predict_corr_knn",
                  "_cocons_hip_vecchia_create_grouped_corr_knn", ".cocons.hip.vecchia.neighbours.corr.pred",
                  ".cocons.hip.vecchia.predict.corr.knn", ".cocons.hip.vecchia.create.grouped.corr.knn"):
        assert entry in doc, entry
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ .*4ag", design, re.M)
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in ("test_corr_knn_pred_reference.py", "test_corr_knn_pred_abi.py", "test_gpu_corr_knn_pred.py",
                 "test_gpu_vecchia_corr_predict.py", "test_gpu_vecchia_grouped_corr.py", "test_glue_vecchia_corr_pred.py",
                 "vecchia_corr_pred_var.py"):
        assert name in readme, name
