"""The expected information at the boundary, without a GPU: cocons_fisher_dense is declared, bound and exported, bad calls
are refused with -1 and a message naming the entry before any HIP call (outputs untouched), and the R glue registers the
entry with its arity and the R wrapper calls it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int\s+cocons_fisher_dense\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int ndir,\s*const double \*dirs,\s*"
        r"double \*info,\s*double \*info_mean\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    assert re.search(DECL, open(os.path.join(ROOT, "include", "cocons_hip.h")).read())
    assert "cocons_fisher_dense" in _lib.SIGNATURES and len(_lib.SIGNATURES["cocons_fisher_dense"][1]) == 6
    assert hasattr(L, "cocons_fisher_dense")
    assert L.cocons_abi_version() == 1


def test_bad_calls_are_refused_without_the_gpu():
    import ctypes
    from cocons_amd import _lib
    L = _lib.load()
    p = 3
    th, dirs = np.zeros(6 * p), np.ones((2, 6 * p))
    info, im = np.full(4, 7.0), np.full(p * p, 7.0)
    assert L.cocons_fisher_dense(None, _dp(th), 2, _dp(dirs), _dp(info), _dp(im)) == -1
    msg = _lib.last_error()
    assert msg.startswith("cocons_fisher_dense:") and "null fit handle" in msg, msg
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the arguments are checked first
    for args in ((None, _dp(dirs), _dp(info)), (_dp(th), None, _dp(info)), (_dp(th), _dp(dirs), None)):
        assert L.cocons_fisher_dense(bogus, args[0], 2, args[1], args[2], _dp(im)) == -1
        assert _lib.last_error().startswith("cocons_fisher_dense: null argument")
    for nd in (0, -1, 7 * _lib.P_MAX + 1):
        assert L.cocons_fisher_dense(bogus, _dp(th), nd, _dp(dirs), _dp(info), _dp(im)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_fisher_dense:") and "ndir" in msg, msg
    assert np.all(info == 7.0) and np.all(im == 7.0)


def test_glue_registers_fisher_entry_and_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_fisher") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.fisher <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_fisher`" in m.group(2)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_fisher_dense", ".cocons.hip.fisher", "getCIs", "getModHess"):
        assert entry in doc
