"""The REML fit's expected information at the boundary, without a GPU: cocons_fisher_reml is declared, bound and exported,
bad calls are refused with -1 and a message naming the entry before any HIP call (info untouched), the R glue registers the
entry with its arity, the R wrapper calls it and INTEGRATION.md names it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int\s+cocons_fisher_reml\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int ndir,\s*const double \*dirs,\s*"
        r"double \*info\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    assert re.search(DECL, open(os.path.join(ROOT, "include", "cocons_hip.h")).read())
    assert "cocons_fisher_reml" in _lib.SIGNATURES and len(_lib.SIGNATURES["cocons_fisher_reml"][1]) == 5
    assert hasattr(L, "cocons_fisher_reml")
    assert L.cocons_abi_version() == 1


def test_bad_calls_are_refused_without_the_gpu():
    import ctypes
    from cocons_amd import _lib
    L = _lib.load()
    p = 3
    th, dirs = np.zeros(6 * p), np.ones((2, 6 * p))
    info = np.full(4, 7.0)
    assert L.cocons_fisher_reml(None, _dp(th), 2, _dp(dirs), _dp(info)) == -1
    msg = _lib.last_error()
    assert msg.startswith("cocons_fisher_reml:") and "null fit handle" in msg, msg
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the arguments are checked first
    for args in ((None, _dp(dirs), _dp(info)), (_dp(th), None, _dp(info)), (_dp(th), _dp(dirs), None)):
        assert L.cocons_fisher_reml(bogus, args[0], 2, args[1], args[2]) == -1
        assert _lib.last_error().startswith("cocons_fisher_reml: null argument")
    for nd in (0, -1, 7 * _lib.P_MAX + 1):
        assert L.cocons_fisher_reml(bogus, _dp(th), nd, _dp(dirs), _dp(info)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_fisher_reml:") and "ndir" in msg, msg
    assert np.all(info == 7.0)


def test_host_layer_is_exported():
    import cocons_amd as ca
    from cocons_amd import host
    assert ca.getFisher_reml is host.getFisher_reml
    assert callable(ca.CoconsFit.fisher_reml_core)


def test_glue_registers_entry_r_wrapper_calls_it_and_the_document_names_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_fisher_reml") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.fisher_reml <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_fisher_reml`" in m.group(2)
    assert [a.strip() for a in m.group(1).split(",")] == ["fit", "theta", "par.pos", "safe = TRUE"]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_fisher_reml", ".cocons.hip.fisher_reml", "_cocons_hip_fisher_reml"):
        assert entry in doc
