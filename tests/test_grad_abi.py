"""The analytic gradient at the boundary, without a GPU: cocons_neg2loglik_grad_dense and the two diagnostics are declared,
bound and exported, bad calls are refused with -1 and a message naming the entry before any HIP call (outputs untouched),
and the R glue registers the entry with its arity and the R wrapper calls it."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_neg2loglik_grad_dense": (
        os.path.join("include", "cocons_hip.h"), "SIGNATURES",
        r"int\s+cocons_neg2loglik_grad_dense\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
        r"double \*sum_logliks,\s*double \*parts,\s*double \*grad_theta,\s*double \*grad_mean\s*\)\s*;", 7),
    "cocons_debug_sigma_inverse": (
        os.path.join("include", "cocons_hip_diag.h"), "DIAG_SIGNATURES",
        r"int\s+cocons_debug_sigma_inverse\s*\(\s*struct cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*double \*out_nxn\s*\)\s*;",
        3),
    "cocons_debug_matern_grad": (
        os.path.join("include", "cocons_hip_diag.h"), "DIAG_SIGNATURES",
        r"int\s+cocons_debug_matern_grad\s*\(\s*int n,\s*const double \*nu,\s*const double \*u,\s*double \*out3n\s*\)\s*;", 4),
}


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    for name, (hdr, table, pat, nargs) in DECLS.items():
        assert re.search(pat, open(os.path.join(ROOT, hdr)).read()), name
        sig = getattr(_lib, table)
        assert name in sig and len(sig[name][1]) == nargs, name
        assert hasattr(L, name)
    assert L.cocons_abi_version() == 1


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p = 3
    th, mean = np.zeros(6 * p), np.zeros(p)
    val = ctypes.c_double(7.0)
    parts, gt, gm = np.full(2, 7.0), np.full(6 * p, 7.0), np.full(p, 7.0)
    out = np.full(9, 7.0)
    assert L.cocons_neg2loglik_grad_dense(None, _dp(th), _dp(mean), ctypes.byref(val), _dp(parts), _dp(gt), _dp(gm)) == -1
    msg = _lib.last_error()
    assert msg.startswith("cocons_neg2loglik_grad_dense:") and "null fit handle" in msg, msg
    assert L.cocons_debug_sigma_inverse(None, _dp(th), _dp(out)) == -1
    msg = _lib.last_error()
    assert msg.startswith("cocons_debug_sigma_inverse:") and "null fit handle" in msg, msg
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the pointer arguments are checked first
    for args in ((None, _dp(mean)), (_dp(th), None)):
        assert L.cocons_neg2loglik_grad_dense(bogus, args[0], args[1], ctypes.byref(val), _dp(parts), _dp(gt), _dp(gm)) == -1
        assert _lib.last_error().startswith("cocons_neg2loglik_grad_dense: null argument")
    assert L.cocons_neg2loglik_grad_dense(bogus, _dp(th), _dp(mean), None, _dp(parts), _dp(gt), _dp(gm)) == -1
    assert L.cocons_neg2loglik_grad_dense(bogus, _dp(th), _dp(mean), ctypes.byref(val), _dp(parts), None, _dp(gm)) == -1
    assert L.cocons_neg2loglik_grad_dense(bogus, _dp(th), _dp(mean), ctypes.byref(val), _dp(parts), _dp(gt), None) == -1
    assert _lib.last_error().startswith("cocons_neg2loglik_grad_dense: null argument")
    assert L.cocons_debug_sigma_inverse(bogus, _dp(th), None) == -1
    assert _lib.last_error().startswith("cocons_debug_sigma_inverse: null argument")
    nu, u, o3 = np.ones(2), np.ones(2), np.full(6, 7.0)
    assert L.cocons_debug_matern_grad(0, _dp(nu), _dp(u), _dp(o3)) == -1
    assert L.cocons_debug_matern_grad(2, _dp(nu), _dp(u), None) == -1
    assert _lib.last_error().startswith("cocons_debug_matern_grad: bad argument")
    assert val.value == 7.0 and np.all(parts == 7.0) and np.all(gt == 7.0) and np.all(gm == 7.0)
    assert np.all(out == 7.0) and np.all(o3 == 7.0)


def test_glue_registers_grad_entry_and_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_neg2loglik_grad") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.neg2loglik\.grad <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_neg2loglik_grad`" in m.group(2)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_neg2loglik_grad_dense", ".cocons.hip.neg2loglik.grad"):
        assert entry in doc
