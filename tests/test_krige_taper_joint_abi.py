"""Joint prediction for tapered fits at the boundary, without a GPU: the C ABI declares and exports
cocons_krige_taper_joint / _joint_bytes, the ctypes binding carries them, every bad call that needs no handle is refused
with -1 and a message starting with the entry's name with the outputs untouched, the R glue registers the entry with its
arity and the R wrapper calls it, and the host layer exports the two functions and the two methods."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_krige_taper_joint": (r"int\s+cocons_krige_taper_joint\s*\(\s*cocons_fit\s*\*\s*fit,\s*int m,\s*"
                                 r"const double \*locs_pred,\s*const double \*X_pred,\s*int nnz_pred,\s*"
                                 r"const int \*colindices_pred,\s*const int \*rowpointers_pred,\s*"
                                 r"const double \*taper_entries_pred,\s*const double \*locs_unobs,\s*int nnz_uu,\s*"
                                 r"const int \*colindices_uu,\s*const int \*rowpointers_uu,\s*const double \*taper_entries_uu,\s*"
                                 r"double \*stochastic,\s*double \*cov,\s*int nsim,\s*const double \*iiderrors,\s*"
                                 r"double \*sims\s*\)\s*;", 18),
    "cocons_krige_taper_joint_bytes": (r"int\s+cocons_krige_taper_joint_bytes\s*\(\s*cocons_fit\s*\*\s*fit,\s*int m,\s*int nsim,\s*"
                                       r"long long \*bytes\s*\)\s*;", 4),
}


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cocons_hip.h")).read(), flags=re.S)     # comments out
    L = _lib.load()
    for name, (pat, nargs) in DECLS.items():
        assert re.search(pat, h), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(L, name)
    assert L.cocons_abi_version() == 1


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    m, p, nsim = 3, 3, 2
    lp, Xp = np.zeros(m * 2), np.zeros(m * p)
    ci, rp, te = np.array([1, 2, 1], dtype=np.int32), np.array([1, 3, 3, 4], dtype=np.int32), np.ones(3)
    cu, ru, tu = np.array([1, 1, 2, 3], dtype=np.int32), np.array([1, 2, 4, 5], dtype=np.int32), np.ones(4)
    st, cov, sims = np.full(m, 7.0), np.full(m * m, 7.0), np.full(m * nsim, 7.0)
    E = np.zeros(m * nsim)
    nbytes = ctypes.c_longlong(9)

    def joint(m_=m, lp_=lp, Xp_=Xp, rp_=rp, ru_=ru, st_=st, nsim_=nsim, E_=E, sims_=sims):
        return L.cocons_krige_taper_joint(None, m_, _dp(lp_), _dp(Xp_), 3, _ip(ci), _ip(rp_), _dp(te), None, 4, _ip(cu), _ip(ru_),
                                          _dp(tu), _dp(st_), _dp(cov), nsim_, _dp(E_), _dp(sims_))

    who = "cocons_krige_taper_joint:"
    for kw, what in ((dict(), "null fit handle"), (dict(m_=0), "m = 0"), (dict(m_=-2), "m = -2"), (dict(lp_=None), "null"),
                     (dict(Xp_=None), "null"), (dict(st_=None), "null"), (dict(rp_=None), "null"), (dict(ru_=None), "null"),
                     (dict(nsim_=-1), "nsim = -1"), (dict(E_=None), "null iiderrors or sims"),
                     (dict(sims_=None), "null iiderrors or sims")):
        assert joint(**kw) == -1, kw
        msg = _lib.last_error()
        assert msg.startswith(who) and what in msg, (kw, msg)
    assert joint(nsim_=0, E_=None, sims_=None) == -1 and "null fit handle" in _lib.last_error()     # no draws: no need of them
    for args, what in (((None, m, 0), "null fit handle"), ((None, 0, 0), "m = 0"), ((None, m, -1), "nsim = -1")):
        assert L.cocons_krige_taper_joint_bytes(*args, ctypes.byref(nbytes)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_krige_taper_joint_bytes:") and what in msg, msg
    assert L.cocons_krige_taper_joint_bytes(None, m, 0, None) == -1
    assert _lib.last_error().startswith("cocons_krige_taper_joint_bytes:")
    assert np.all(st == 7.0) and np.all(cov == 7.0) and np.all(sims == 7.0) and nbytes.value == 9


def test_glue_registers_the_entry_and_the_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_krige_taper_joint") == 8
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.krige\.taper\.joint <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_krige_taper_joint`" in m.group(2)
    for arg in ("fit", "newlocs", "X_pred", "pred_taper", "uu_taper", "locs_unobs = NULL", "iiderrors = NULL", "cov = TRUE"):
        assert arg in m.group(1), arg
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_krige_taper_joint", "_cocons_hip_krige_taper_joint", ".cocons.hip.krige.taper.joint"):
        assert entry in doc, entry


def test_host_layer_exports_the_functions_and_the_methods():
    import cocons_amd as ca
    for name in ("cocoPredict_sparse_joint", "cocoSim_cond_sparse_held"):
        assert callable(getattr(ca, name)) and callable(getattr(ca.host, name)), name
    for name in ("krige_taper_joint_core", "krige_taper_joint_bytes"):
        assert callable(getattr(ca.CoconsTaperFit, name)), name
        assert not hasattr(ca.CoconsFit, name), name
    assert issubclass(ca.KrigeJointNotPositiveDefinite, ca.CoconsHipError)
