"""The Profile / REML gradients at the boundary, without a GPU: cocons_neg2loglik_profile_grad and cocons_neg2loglik_reml_grad
are declared, bound and exported, bad calls are refused with -1 and a message naming the entry before any HIP call (outputs
untouched), the R glue registers both entries with their arities, the R wrappers call them, INTEGRATION.md names them, and
the host layer exports the two functions and the two CoconsFit methods."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_neg2loglik_profile_grad": (
        r"int\s+cocons_neg2loglik_profile_grad\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*"
        r"double \*sum_logliks,\s*double \*parts,\s*double \*grad_theta\s*\)\s*;", 5),
    "cocons_neg2loglik_reml_grad": (
        r"int\s+cocons_neg2loglik_reml_grad\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int rank,\s*"
        r"double \*sum_logliks,\s*double \*parts,\s*double \*grad_theta\s*\)\s*;", 6),
}


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    for name, (pat, nargs) in DECLS.items():
        assert re.search(pat, header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name)
    assert L.cocons_abi_version() == 1


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p = 3
    th = np.zeros(6 * p)
    val = ctypes.c_double(7.0)
    parts, gt = np.full(8, 7.0), np.full(6 * p, 7.0)
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the pointer arguments are checked first

    def profile(h, t, v, g):
        return L.cocons_neg2loglik_profile_grad(h, t, v, _dp(parts), g)

    def reml(h, t, v, g):
        return L.cocons_neg2loglik_reml_grad(h, t, 3, v, _dp(parts), g)

    for name, call in (("cocons_neg2loglik_profile_grad", profile), ("cocons_neg2loglik_reml_grad", reml)):
        assert call(None, _dp(th), ctypes.byref(val), _dp(gt)) == -1
        msg = _lib.last_error()
        assert msg.startswith(name + ":") and "null fit handle" in msg, msg
        for args in ((None, ctypes.byref(val), _dp(gt)), (_dp(th), None, _dp(gt)), (_dp(th), ctypes.byref(val), None)):
            assert call(bogus, *args) == -1
            assert _lib.last_error().startswith(name + ": null argument"), _lib.last_error()
    assert val.value == 7.0 and np.all(parts == 7.0) and np.all(gt == 7.0)


def test_glue_registers_both_entries_and_r_wrappers_call_them():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_neg2loglik_profile_grad") == 2
    assert R.L.stub_registered_arity(b"_cocons_hip_neg2loglik_reml_grad") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry in (("GetNeg2loglikelihoodProfileGrad", "_cocons_hip_neg2loglik_profile_grad"),
                      ("GetNeg2loglikelihoodREMLGrad", "_cocons_hip_neg2loglik_reml_grad")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
        assert ".cocons.hip.profile.grad" in m.group(2)
        assert "safe = TRUE" in m.group(1) and "fit = NULL" in m.group(1)
    helper = re.search(r"\.cocons\.hip\.profile\.grad <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert helper and ".cocons.hip.getPen.grad" in helper.group(2) and ".cocons.hip.diff.grad" in helper.group(2)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_neg2loglik_profile_grad", "cocons_neg2loglik_reml_grad", "_cocons_hip_neg2loglik_profile_grad",
                  "_cocons_hip_neg2loglik_reml_grad", "GetNeg2loglikelihoodProfileGrad", "GetNeg2loglikelihoodREMLGrad"):
        assert entry in doc, entry


def test_host_exports():
    import cocons_amd as ca
    from cocons_amd import host
    for name in ("GetNeg2loglikelihoodProfile_grad", "GetNeg2loglikelihoodREML_grad"):
        assert callable(getattr(host, name)) and getattr(ca, name) is getattr(host, name)
    for name in ("neg2loglik_profile_grad_core", "neg2loglik_reml_grad_core"):
        assert callable(getattr(host.CoconsFit, name))
