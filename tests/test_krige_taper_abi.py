"""Tapered kriging from a held band factor at the boundary, without a GPU: the C ABI declares and exports
cocons_krige_taper_prepare / _apply / _release / _info, the ctypes binding carries them, bad calls are refused with -1 and
a message naming the entry point before any HIP call, the R glue registers the three entries with their arities and the R
wrappers call them, and the host layer exports the function and the four methods."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_krige_taper_prepare": (r"int\s+cocons_krige_taper_prepare\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*"
                                   r"const double \*mean,\s*int z_col,\s*int max_rows\s*\)\s*;", 5),
    "cocons_krige_taper_apply": (r"int\s+cocons_krige_taper_apply\s*\(\s*cocons_fit\s*\*\s*fit,\s*int m,\s*"
                                 r"const double \*locs_pred,\s*const double \*X_pred,\s*int nnz_pred,\s*"
                                 r"const int \*colindices_pred,\s*const int \*rowpointers_pred,\s*"
                                 r"const double \*taper_entries_pred,\s*double \*stochastic,\s*double \*quadform\s*\)\s*;", 10),
    "cocons_krige_taper_release": (r"int\s+cocons_krige_taper_release\s*\(\s*cocons_fit\s*\*\s*fit\s*\)\s*;", 1),
    "cocons_krige_taper_info": (r"int\s+cocons_krige_taper_info\s*\(\s*cocons_fit\s*\*\s*fit,\s*long long \*out6\s*\)\s*;", 2),
}


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    for name, (pat, nargs) in DECLS.items():
        assert re.search(pat, h), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(L, name)
    assert L.cocons_abi_version() == 1


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    m, p = 3, 3
    th, mean = np.zeros(6 * p), np.zeros(p)
    lp, Xp = np.zeros(m * 2), np.zeros(m * p)
    ci, rp, te = np.array([1, 2, 1], dtype=np.int32), np.array([1, 3, 3, 4], dtype=np.int32), np.ones(3)
    st, qf = np.full(m, 7.0), np.full(m, 7.0)
    info = (ctypes.c_longlong * 6)(9, 9, 9, 9, 9, 9)

    def apply(h=None, m_=m, nnz=3, ci_=ci, rp_=rp, te_=te, st_=st, qf_=qf):
        return L.cocons_krige_taper_apply(h, m_, _dp(lp), _dp(Xp), nnz, None if ci_ is None else _ip(ci_),
                                          None if rp_ is None else _ip(rp_), None if te_ is None else _dp(te_),
                                          None if st_ is None else _dp(st_), None if qf_ is None else _dp(qf_))

    cases = (
        ("cocons_krige_taper_prepare", lambda: L.cocons_krige_taper_prepare(None, _dp(th), _dp(mean), 0, 0)),
        ("cocons_krige_taper_apply", apply),
        ("cocons_krige_taper_release", lambda: L.cocons_krige_taper_release(None)),
        ("cocons_krige_taper_info", lambda: L.cocons_krige_taper_info(None, info)),
    )
    for name, call in cases:
        assert call() == -1
        msg = _lib.last_error()
        assert msg.startswith(name + ":") and "null fit handle" in msg, msg
    # the arguments of apply are checked before the handle: a negative m, a negative nnz and NULL pointers
    for kw in (dict(m_=-1), dict(nnz=-1), dict(st_=None), dict(qf_=None), dict(rp_=None), dict(ci_=None), dict(te_=None)):
        assert apply(**kw) == -1
        assert _lib.last_error().startswith("cocons_krige_taper_apply: bad argument"), (kw, _lib.last_error())
    assert np.all(st == 7.0) and np.all(qf == 7.0) and list(info) == [9] * 6


def test_glue_registers_krige_taper_entries_and_r_wrappers_call_them():
    from test_glue_exec import RStub
    R = RStub()
    for name, arity in (("_cocons_hip_krige_taper_prepare", 5), ("_cocons_hip_krige_taper", 6),
                        ("_cocons_hip_krige_taper_release", 1)):
        assert R.L.stub_registered_arity(name.encode()) == arity, name
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry in ((r"\.cocons\.hip\.krige\.taper\.prepare", "_cocons_hip_krige_taper_prepare"),
                      (r"\.cocons\.hip\.krige\.taper", "_cocons_hip_krige_taper"),
                      (r"\.cocons\.hip\.krige\.taper\.release", "_cocons_hip_krige_taper_release")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_krige_taper_prepare", "cocons_krige_taper_apply", "_cocons_hip_krige_taper"):
        assert entry in doc


def test_host_layer_exports_the_function_and_the_methods():
    import cocons_amd as ca
    assert callable(ca.cocoPredict_sparse_chunked)
    for name in ("krige_taper_prepare", "krige_taper_core", "krige_taper_release", "krige_taper_info"):
        assert callable(getattr(ca.CoconsTaperFit, name)), name
    # the dense names stay what they were on a taper handle: inherited, refusing
    assert ca.CoconsTaperFit.krige_prepare is ca.CoconsFit.krige_prepare
