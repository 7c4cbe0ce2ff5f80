"""The taper gradient at the boundary, without a GPU: cocons_neg2loglik_grad_taper and its diagnostic are declared, bound and
exported, bad calls are refused with -1 and a message naming the entry before any HIP call (outputs untouched), the R glue
registers its entry with its arity, the R wrappers call it, INTEGRATION.md names them, and the host layer exports the two
functions and the CoconsTaperFit method."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int\s+cocons_neg2loglik_grad_taper\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
        r"double \*sum_logliks,\s*double \*parts,\s*double \*grad_theta,\s*double \*grad_quad,\s*double \*grad_mean\s*\)\s*;")
DIAG_DECL = (r"int\s+cocons_debug_taper_selinv\s*\(\s*struct cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*double \*out_nnz,\s*"
             r"long long \*bytes_out\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    assert re.search(DECL, open(os.path.join(ROOT, "include", "cocons_hip.h")).read())
    assert re.search(DIAG_DECL, open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read())
    assert len(_lib.SIGNATURES["cocons_neg2loglik_grad_taper"][1]) == 8
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_taper_selinv"][1]) == 4
    assert hasattr(L, "cocons_neg2loglik_grad_taper") and hasattr(L, "cocons_debug_taper_selinv")
    assert L.cocons_abi_version() == 1


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p = 3
    name = "cocons_neg2loglik_grad_taper"
    th, mean = np.zeros(6 * p), np.zeros(p)
    val = ctypes.c_double(7.0)
    parts, gt, gq, gm = np.full(3, 7.0), np.full(6 * p, 7.0), np.full(6 * p, 7.0), np.full(p, 7.0)
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the pointer arguments are checked first
    good = [_dp(th), _dp(mean), ctypes.byref(val), _dp(parts), _dp(gt), _dp(gq), _dp(gm)]
    assert L.cocons_neg2loglik_grad_taper(None, *good) == -1
    msg = _lib.last_error()
    assert msg.startswith(name + ":") and "null fit handle" in msg, msg
    for k in (0, 1, 2, 4, 6):              # theta, mean, sum_logliks, grad_theta, grad_mean (parts and grad_quad may be null)
        args = list(good)
        args[k] = None
        assert L.cocons_neg2loglik_grad_taper(bogus, *args) == -1
        assert _lib.last_error().startswith(name + ": null argument"), _lib.last_error()
    assert val.value == 7.0 and all(np.all(a == 7.0) for a in (parts, gt, gq, gm))
    name = "cocons_debug_taper_selinv"
    nb = ctypes.c_longlong(7)
    assert L.cocons_debug_taper_selinv(None, _dp(th), _dp(gt), ctypes.byref(nb)) == -1
    assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
    for args in ((None, _dp(gt)), (_dp(th), None)):
        assert L.cocons_debug_taper_selinv(bogus, *args, ctypes.byref(nb)) == -1
        assert _lib.last_error().startswith(name + ": null argument"), _lib.last_error()
    assert nb.value == 7 and np.all(gt == 7.0)


def test_glue_registers_the_entry_and_r_wrappers_call_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_neg2loglik_taper_grad") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.neg2loglik\.taper\.grad <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_neg2loglik_taper_grad`" in m.group(2)
    for fn in ("GetNeg2loglikelihoodTaperGrad", "GetNeg2loglikelihoodTaperProfileGrad"):
        m = re.search(r"\.cocons\.hip\." + fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ".cocons.hip.neg2loglik.taper.grad" in m.group(2), fn
        assert ".cocons.hip.getPen.grad" in m.group(2) and ".cocons.hip.diff.grad" in m.group(2)
        assert "safe = TRUE" in m.group(1)
        if "Profile" in fn:
            assert "theta_list$std.dev[1] <- 0" in m.group(2) and "G$std.dev[1] <- 0" in m.group(2)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_neg2loglik_grad_taper", "_cocons_hip_neg2loglik_taper_grad", ".cocons.hip.neg2loglik.taper.grad",
                  ".cocons.hip.GetNeg2loglikelihoodTaperGrad", ".cocons.hip.GetNeg2loglikelihoodTaperProfileGrad"):
        assert entry in doc, entry


def test_host_exports():
    import cocons_amd as ca
    from cocons_amd import host
    for name in ("GetNeg2loglikelihoodTaper_grad", "GetNeg2loglikelihoodTaperProfile_grad"):
        assert callable(getattr(host, name)) and getattr(ca, name) is getattr(host, name)
    assert host.CoconsTaperFit.neg2loglik_grad_core is not host.CoconsFit.neg2loglik_grad_core
