"""The Vecchia neighbours by model correlation at the boundary, without a GPU: the header declares
cocons_vecchia_neighbours_corr and cocons_fit_create_vecchia_corr_knn and states their rule, the library exports them and the
ctypes binding carries them; every bad call is refused with -1 (NULL) and a message naming the entry before any HIP call (a HIP
call without a device fails with another code and another message), with the output untouched; the host layer exports the
restatement and the methods, and the documents name the entries.  (The refusals that need a live handle -- another kind of
handle, a theta that is not finite on cocons_vecchia_neighbours_corr -- are in test_gpu_corr_knn.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_vecchia_neighbours_corr": (r"int\s+cocons_vecchia_neighbours_corr\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*"
                                       r"int m_cand,\s*int hops,\s*int m,\s*int \*nn_out[^)]*\)\s*;", 6),
    "cocons_fit_create_vecchia_corr_knn": (r"cocons_fit\s*\*\s*cocons_fit_create_vecchia_corr_knn\s*\(\s*int n,\s*int p,\s*int r,\s*"
                                           r"const double \*locs,\s*const double \*X,\s*const double \*z,\s*"
                                           r"const double \*smooth_limits,\s*int device,\s*const double \*theta,\s*int m_cand,\s*"
                                           r"int hops,\s*int m\s*\)\s*;", 12),
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
    for phrase in ("rho descending, index ascending", "fl(v / fl(sqrt(fl(d_i d_j))))", "63 + 63^2 = 4032",
                   "first m columns", "ranks all its predecessors", "failing-block convention"):
        assert phrase in h, phrase
    d = open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read()
    assert re.search(r"int\s+cocons_debug_knn_corr_phases\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int m_cand,\s*"
                     r"int hops,\s*int m,\s*double \*ms3\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_knn_corr_phases"][1]) == 6 and hasattr(L, "cocons_debug_knn_corr_phases")
    ms = np.full(3, -7.0)
    assert L.cocons_debug_knn_corr_phases(ctypes.c_void_p(1), _dp(np.zeros(6)), 5, 3, 3, _dp(ms)) == -1
    assert _lib.last_error().startswith("cocons_debug_knn_corr_phases: hops = 3") and np.all(ms == -7.0)
    assert L.cocons_abi_version() == 1          # the entries add to the ABI and change nothing in it


def test_neighbours_corr_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    name = "cocons_vecchia_neighbours_corr"
    theta = np.zeros(6)
    nn = np.full(4 * 64, -7, dtype=np.int32)
    fake = ctypes.c_void_p(1)          # never dereferenced: every case below is refused on its arguments alone

    def call(f=fake, theta_=theta, m_cand=5, hops=2, m=3, nn_=nn):
        return L.cocons_vecchia_neighbours_corr(f, _dp(theta_), m_cand, hops, m, _ip(nn_))

    assert call(f=None) == -1
    assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
    for kw in (dict(theta_=None), dict(nn_=None), dict(m_cand=0), dict(m_cand=64), dict(m_cand=-1), dict(hops=0), dict(hops=3),
               dict(m=0), dict(m=64), dict(m=-5),
               dict(m_cand=5, hops=1, m=6),             # one hop: at most m_cand candidates
               dict(m_cand=1, hops=2, m=3),             # two hops: at most m_cand + m_cand^2
               dict(m_cand=7, hops=2, m=57)):
        assert call(**kw) == -1, kw
        msg = _lib.last_error()
        assert msg.startswith(name + ":") and "null fit handle" not in msg, (kw, msg)
    assert np.all(nn == -7)


def test_create_corr_knn_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    name = "cocons_fit_create_vecchia_corr_knn"
    n, p = 4, 2
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    bad = locs.copy(); bad[1] = np.nan
    X, z, sl, theta = np.ones(n * p), np.ones(n), np.array([0.5, 2.5]), np.zeros(6 * p)
    nan_theta = theta.copy(); nan_theta[7] = np.nan
    inf_theta = theta.copy(); inf_theta[0] = -np.inf

    def create(n_=n, locs_=locs, X_=X, z_=z, sl_=sl, theta_=theta, m_cand=3, hops=2, m=2, p_=p, r=1):
        return L.cocons_fit_create_vecchia_corr_knn(n_, p_, r, _dp(locs_), _dp(X_), _dp(z_), _dp(sl_), 0, _dp(theta_), m_cand,
                                                    hops, m)

    for kw in (dict(locs_=None), dict(X_=None), dict(z_=None), dict(sl_=None), dict(theta_=None), dict(n_=0), dict(p_=0), dict(r=0),
               dict(locs_=bad), dict(theta_=nan_theta), dict(theta_=inf_theta), dict(m_cand=0), dict(m_cand=64), dict(hops=0),
               dict(hops=3), dict(m=0), dict(m=64), dict(m_cand=3, hops=1, m=4), dict(m_cand=2, hops=2, m=7)):
        assert not create(**kw), kw
        assert _lib.last_error().startswith(name + ":"), (kw, _lib.last_error())


def test_host_layer_exports_the_restatement_and_the_methods():
    import cocons_amd as ca
    assert list(inspect.signature(ca.vecchia_neighbours_corr).parameters) == ["S", "nn_cand", "m", "hops"]
    sig = inspect.signature(ca.CoconsVecchiaFit.neighbours_corr)
    assert list(sig.parameters)[1:] == ["theta_list", "m", "m_cand", "hops"]
    assert sig.parameters["m_cand"].default is None and sig.parameters["hops"].default == 2
    for name in ("from_corr_knn", "from_maxmin_corr"):
        sig = inspect.signature(getattr(ca.CoconsVecchiaFit, name))
        assert list(sig.parameters) == ["locs", "x_covariates", "z", "smooth_limits", "theta_list", "m", "m_cand", "hops", "device"]
    # the existing constructors keep their signatures
    assert list(inspect.signature(ca.CoconsVecchiaFit.from_knn).parameters) == ["locs", "x_covariates", "z", "smooth_limits", "m", "device"]
    assert list(inspect.signature(ca.CoconsVecchiaFit.from_maxmin).parameters) == ["locs", "x_covariates", "z", "smooth_limits", "m", "device"]


def test_the_documents_name_the_entries():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_vecchia_neighbours_corr", "cocons_fit_create_vecchia_corr_knn", "_cocons_hip_vecchia_neighbours_corr",
                  "_cocons_hip_vecchia_create_corr_knn", ".cocons.hip.vecchia.neighbours.corr", ".cocons.hip.vecchia.create.corr.knn"):
        assert entry in doc, entry
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ .*4af", design, re.M)
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in ("test_corr_knn_reference.py", "test_gpu_corr_knn.py", "test_gpu_vecchia_corr_handle.py", "vecchia_corr_kl.py"):
        assert name in readme, name
