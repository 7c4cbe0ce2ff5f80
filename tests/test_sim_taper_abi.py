"""cocoSim's sparse branch (R/sim.R:177-217) at the boundary, without a GPU: the C ABI declares and exports
cocons_sim_taper / cocons_fit_taper_order, the ctypes binding carries them, a NULL handle is refused before any HIP
call, and the R glue registers `_cocons_hip_sim_taper` with its arity and the R wrapper calls it."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "cocons_hip.h")).read()


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = _header()
    assert re.search(r"int\s+cocons_sim_taper\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,"
                     r"\s*int nsim,\s*const double \*iiderrors,\s*const int \*pivot,\s*double \*out\s*\)\s*;", h)
    assert re.search(r"int\s+cocons_fit_taper_order\s*\(\s*cocons_fit\s*\*\s*fit,\s*int \*pivot_out\s*\)\s*;", h)
    for name, nargs in (("cocons_sim_taper", 7), ("cocons_fit_taper_order", 2)):
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    L = _lib.load()
    assert L.cocons_abi_version() == 1
    assert hasattr(L, "cocons_sim_taper") and hasattr(L, "cocons_fit_taper_order")


def test_null_handle_is_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    n, nsim = 4, 2
    th = np.zeros(6 * 3)
    mean = np.zeros(3)
    E = np.zeros(n * nsim)
    out = np.full(n * nsim, 7.0)
    piv = np.arange(1, n + 1, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)                        # noqa: E731
    ip = piv.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    rc = L.cocons_sim_taper(None, dp(th), dp(mean), nsim, dp(E), None, dp(out))
    assert rc < 0 and "null fit handle" in _lib.last_error()
    rc = L.cocons_sim_taper(None, dp(th), dp(mean), nsim, dp(E), ip, dp(out))
    assert rc < 0 and "null fit handle" in _lib.last_error()
    assert np.all(out == 7.0)
    rc = L.cocons_fit_taper_order(None, ip)
    assert rc < 0 and "null fit handle" in _lib.last_error()


def test_glue_registers_sim_taper_and_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_sim_taper") == 5
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.sim\.taper <- function\(fit, theta_list, iiderrors, pivot = NULL\) \{(.*?)\n\}", src, re.S)
    assert m and "_cocons_hip_sim_taper" in m.group(1)
    assert "_cocons_hip_sim_taper" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
