"""Cross-validated predictions at the boundary, without a GPU: cocons_cv_dense and cocons_cv_taper are declared, bound and
exported, bad calls are refused with -1 and a message naming the entry before any HIP call (outputs untouched), the host layer
is exported, the R glue registers both entries with their arities, the R wrappers exist with their argument lists and
INTEGRATION.md names the entries."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL_DENSE = (r"int\s+cocons_cv_dense\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
              r"int nfold,\s*const int \*fold,\s*double \*resid,\s*double \*var\s*\)\s*;")
DECL_TAPER = (r"int\s+cocons_cv_taper\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
              r"double \*resid,\s*double \*var\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    assert re.search(DECL_DENSE, header) and re.search(DECL_TAPER, header)
    assert len(_lib.SIGNATURES["cocons_cv_dense"][1]) == 7 and len(_lib.SIGNATURES["cocons_cv_taper"][1]) == 5
    assert hasattr(L, "cocons_cv_dense") and hasattr(L, "cocons_cv_taper")
    assert L.cocons_abi_version() == 1


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p, n = 3, 5
    th, mean = np.zeros(6 * p), np.zeros(p)
    resid, var = np.full(n, 7.0), np.full(n, 7.0)
    fold = np.zeros(n, dtype=np.int32)
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the arguments are checked first
    assert L.cocons_cv_dense(None, _dp(th), _dp(mean), 0, None, _dp(resid), _dp(var)) == -1
    assert _lib.last_error() == "cocons_cv_dense: null fit handle"
    assert L.cocons_cv_taper(None, _dp(th), _dp(mean), _dp(resid), _dp(var)) == -1
    assert _lib.last_error() == "cocons_cv_taper: null fit handle"
    good = [_dp(th), _dp(mean), _dp(resid), _dp(var)]
    for hole in range(4):
        a = [None if k == hole else good[k] for k in range(4)]
        assert L.cocons_cv_dense(bogus, a[0], a[1], 0, None, a[2], a[3]) == -1
        assert _lib.last_error().startswith("cocons_cv_dense: null argument")
        assert L.cocons_cv_taper(bogus, *a) == -1
        assert _lib.last_error().startswith("cocons_cv_taper: null argument")
    for nfold, fp, word in ((-1, _ip(fold), "nfold"), (-1, None, "nfold"), (0, _ip(fold), "disagree"), (2, None, "disagree")):
        assert L.cocons_cv_dense(bogus, good[0], good[1], nfold, fp, good[2], good[3]) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_cv_dense:") and word in msg, msg
    assert np.all(resid == 7.0) and np.all(var == 7.0)


def test_host_layer_is_exported():
    import cocons_amd as ca
    from cocons_amd import host
    for name in ("cocoCV_dense", "cocoCV_sparse", "getLogScore", "getCRPS"):
        assert getattr(ca, name) is getattr(host, name)
    assert callable(ca.CoconsFit.cv_core) and callable(ca.CoconsTaperFit.cv_core)
    assert ca.CoconsTaperFit.cv_core is not ca.CoconsFit.cv_core


def test_glue_registers_entries_r_wrappers_exist_and_the_document_names_them():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_cv") == 4
    assert R.L.stub_registered_arity(b"_cocons_hip_cv_taper") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for name, symbol, args in ((r"\.cocons\.hip\.cv", "`_cocons_hip_cv`", ["fit", "theta_list", "fold = NULL", "safe = TRUE"]),
                               (r"\.cocons\.hip\.cv\.taper", "`_cocons_hip_cv_taper`", ["fit", "theta_list", "safe = TRUE"])):
        m = re.search(name + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and symbol in m.group(2), name
        assert [a.strip() for a in m.group(1).split(",")] == args
        assert ".cocons.hip.result" in m.group(2)
    assert "match(fold, unique(fold)) - 1L" in src
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_cv_dense", "cocons_cv_taper", ".cocons.hip.cv", ".cocons.hip.cv.taper", "_cocons_hip_cv", "getCRPS"):
        assert entry in doc
