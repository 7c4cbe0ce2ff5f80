"""Kriging from a held factor at the boundary, without a GPU: the C ABI declares and exports cocons_krige_prepare /
_apply / _release / _info, the ctypes binding carries them, bad calls are refused with -1 and a message naming the entry
point before any HIP call, and the R glue registers the three entries with their arities and the R wrappers call them."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_krige_prepare": (r"int\s+cocons_krige_prepare\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*"
                             r"const double \*mean,\s*int z_col,\s*int max_rows\s*\)\s*;", 5),
    "cocons_krige_apply": (r"int\s+cocons_krige_apply\s*\(\s*cocons_fit\s*\*\s*fit,\s*int m,\s*const double \*locs_pred,\s*"
                           r"const double \*X_pred,\s*double \*stochastic,\s*double \*quadform\s*\)\s*;", 6),
    "cocons_krige_release": (r"int\s+cocons_krige_release\s*\(\s*cocons_fit\s*\*\s*fit\s*\)\s*;", 1),
    "cocons_krige_info": (r"int\s+cocons_krige_info\s*\(\s*cocons_fit\s*\*\s*fit,\s*long long \*out4\s*\)\s*;", 2),
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


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    m, p = 3, 3
    th, mean = np.zeros(6 * p), np.zeros(p)
    lp, Xp = np.zeros(m * 2), np.zeros(m * p)
    st, qf = np.full(m, 7.0), np.full(m, 7.0)
    info = (ctypes.c_longlong * 4)(9, 9, 9, 9)
    cases = (
        ("cocons_krige_prepare", lambda: L.cocons_krige_prepare(None, _dp(th), _dp(mean), 0, 0)),
        ("cocons_krige_apply", lambda: L.cocons_krige_apply(None, m, _dp(lp), _dp(Xp), _dp(st), _dp(qf))),
        ("cocons_krige_release", lambda: L.cocons_krige_release(None)),
        ("cocons_krige_info", lambda: L.cocons_krige_info(None, info)),
    )
    for name, call in cases:
        assert call() == -1
        msg = _lib.last_error()
        assert msg.startswith(name + ":") and "null fit handle" in msg, msg
    # the arguments of apply are checked before the handle: a negative m and a NULL output pointer
    assert L.cocons_krige_apply(None, -1, _dp(lp), _dp(Xp), _dp(st), _dp(qf)) == -1
    assert _lib.last_error().startswith("cocons_krige_apply: bad argument")
    assert L.cocons_krige_apply(None, m, _dp(lp), _dp(Xp), None, _dp(qf)) == -1
    assert _lib.last_error().startswith("cocons_krige_apply: bad argument")
    assert L.cocons_krige_apply(None, m, _dp(lp), _dp(Xp), _dp(st), None) == -1
    assert _lib.last_error().startswith("cocons_krige_apply: bad argument")
    assert np.all(st == 7.0) and np.all(qf == 7.0) and list(info) == [9, 9, 9, 9]


def test_glue_registers_krige_entries_and_r_wrappers_call_them():
    from test_glue_exec import RStub
    R = RStub()
    for name, arity in (("_cocons_hip_krige_prepare", 5), ("_cocons_hip_krige", 3), ("_cocons_hip_krige_release", 1)):
        assert R.L.stub_registered_arity(name.encode()) == arity, name
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry in ((r"\.cocons\.hip\.krige\.prepare", "_cocons_hip_krige_prepare"),
                      (r"\.cocons\.hip\.krige", "_cocons_hip_krige"),
                      (r"\.cocons\.hip\.krige\.release", "_cocons_hip_krige_release")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_krige_prepare", "cocons_krige_apply", "_cocons_hip_krige"):
        assert entry in doc
