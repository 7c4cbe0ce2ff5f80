"""Cross-validation of tapered fits by folds at the boundary, without a GPU: cocons_cv_taper_folds is declared, bound (9
arguments) and exported and the ABI version is still 1; what can be refused without a handle is refused with -1 and a message
naming the entry before any HIP call (outputs untouched); the host signatures, the glue's arity, the R wrapper's argument list
and INTEGRATION.md."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int\s+cocons_cv_taper_folds\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
        r"int nfold,\s*const int \*fold,\s*int max_rows,\s*double \*resid,\s*double \*var,\s*long long \*stats5\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    assert re.search(DECL, header)
    res, args = _lib.SIGNATURES["cocons_cv_taper_folds"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[4] == ctypes.POINTER(ctypes.c_int) and args[8] == ctypes.POINTER(ctypes.c_longlong)
    assert hasattr(L, "cocons_cv_taper_folds")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r" T cocons_cv_taper_folds\b", exported)
    assert L.cocons_abi_version() == 1
    # the leave-one-out entry keeps its signature
    assert len(_lib.SIGNATURES["cocons_cv_taper"][1]) == 5


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p, n = 3, 5
    th, mean = np.zeros(6 * p), np.zeros(p)
    resid, var = np.full(n, 7.0), np.full(n, 7.0)
    stats = (ctypes.c_longlong * 5)(7, 7, 7, 7, 7)
    fold = np.zeros(n, dtype=np.int32)
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the arguments are checked first
    good = [_dp(th), _dp(mean), _dp(resid), _dp(var)]
    assert L.cocons_cv_taper_folds(None, good[0], good[1], 0, None, 0, good[2], good[3], stats) == -1
    assert _lib.last_error() == "cocons_cv_taper_folds: null fit handle"
    for hole in range(4):
        a = [None if k == hole else good[k] for k in range(4)]
        assert L.cocons_cv_taper_folds(bogus, a[0], a[1], 0, None, 0, a[2], a[3], stats) == -1
        assert _lib.last_error().startswith("cocons_cv_taper_folds: null argument")
    for nfold, fp, mr, word in ((-1, _ip(fold), 0, "nfold"), (-1, None, 0, "nfold"), (0, _ip(fold), 0, "disagree"),
                                (2, None, 0, "disagree"), (2, _ip(fold), -1, "max_rows"), (0, None, -128, "max_rows")):
        assert L.cocons_cv_taper_folds(bogus, good[0], good[1], nfold, fp, mr, good[2], good[3], stats) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_cv_taper_folds:") and word in msg, msg
        assert L.cocons_cv_taper_folds(bogus, good[0], good[1], nfold, fp, mr, good[2], good[3], None) == -1
    assert np.all(resid == 7.0) and np.all(var == 7.0) and list(stats) == [7] * 5


def test_host_signatures():
    import cocons_amd as ca
    from cocons_amd import host
    sig = inspect.signature(ca.CoconsTaperFit.cv_core)
    assert list(sig.parameters) == ["self", "theta_list", "fold", "max_rows"]
    assert sig.parameters["fold"].default is None and sig.parameters["max_rows"].default == 0
    sig = inspect.signature(host.cocoCV_sparse)
    assert list(sig.parameters) == ["theta_list", "locs", "X_std", "smooth_limits", "z", "ref_taper", "fit", "fold"]
    assert sig.parameters["fit"].default is None and sig.parameters["fold"].default is None
    assert ca.cocoCV_sparse is host.cocoCV_sparse


def test_glue_arity_r_wrapper_and_the_document():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_cv_taper_folds") == 5
    assert R.L.stub_registered_arity(b"_cocons_hip_cv_taper") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.cv\.taper\.folds <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_cv_taper_folds`" in m.group(2)
    assert [a.strip() for a in m.group(1).split(",")] == ["fit", "theta_list", "fold", "max_rows = 0L", "safe = TRUE"]
    assert ".cocons.hip.result" in m.group(2) and "match(fold, unique(fold)) - 1L" in m.group(2)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_cv_taper_folds", ".cocons.hip.cv.taper.folds", "_cocons_hip_cv_taper_folds"):
        assert entry in doc
