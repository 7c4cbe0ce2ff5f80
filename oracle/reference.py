"""oracle/reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Loader of `oracle/_ref/libcocons_ref.so`: the reference's own src/cocons_full.cpp, src/cocons_taper.cpp
and src/cocons_types.h, compiled unmodified behind oracle/ref_wrap.cpp with the stand-in headers of
oracle/ref_shim/ (oracle/Makefile, target `ref`).  The call signatures mirror oracle/oracle.py, so a test
can hand the same arguments to both and compare bits.  K_nu inside this library is the oracle's
(ref_shim/boost/...); everything around it is the reference's compiled code.

The library exists only where the reference's sources are (REF_SRC, overridable through the
environment variable COCONS_REF_SRC); it is never committed.  Only tests/ and the tools under oracle/
and tests/golden/ may import this module.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from . import oracle as _O

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {}

DEFAULT_REF_SRC = "/root/reference/src"
SOURCES = ("cocons_full.cpp", "cocons_taper.cpp", "cocons_types.h")


def ref_src() -> str:
    return os.environ.get("COCONS_REF_SRC", DEFAULT_REF_SRC)


def have_sources() -> bool:
    return all(os.path.isfile(os.path.join(ref_src(), s)) for s in SOURCES)


def lib_path() -> str:
    return os.path.join(_HERE, "_ref", "libcocons_ref.so")


def available() -> bool:
    """True where the live comparison can run: the library is there, or its sources are (then it is built)."""
    return os.path.isfile(lib_path()) or have_sources()


def build() -> str:
    """Build (or bring up to date) oracle/_ref/libcocons_ref.so where the reference's sources are present;
    where they are not, an existing library is used as it is."""
    _O.build()
    if have_sources():
        subprocess.check_call(["make", "-C", _HERE, "-s", "ref", "REF_SRC=" + ref_src()])
    if not os.path.isfile(lib_path()):
        raise FileNotFoundError("%s is absent and the reference sources are not under %s" % (lib_path(), ref_src()))
    return lib_path()


def lib(path: str | None = None):
    """The loaded library (built first when `path` is not given)."""
    key = path or ""
    if key not in _LIBS:
        _O.lib()        # the oracle's library provides K_nu: same process, same code
        L = ctypes.CDLL(path or build())
        dp = ctypes.POINTER(ctypes.c_double)
        ip = ctypes.POINTER(ctypes.c_int)
        ci = ctypes.c_int
        L.ref_cov_rns.argtypes = [ci, ci, dp, dp, dp, dp, dp]
        L.ref_cov_rns_classic.argtypes = [ci, ci, dp, dp, dp, dp]
        L.ref_cov_rns_pred.argtypes = [ci, ci, ci, dp, dp, dp, dp, dp, dp, dp]
        L.ref_cov_rns_taper.argtypes = [ci, ci, dp, dp, dp, dp, ci, ip, ip, dp]
        L.ref_cov_rns_taper_pred.argtypes = [ci, ci, ci, dp, dp, dp, dp, dp, dp, ci, ip, ip, dp]
        L.ref_sumsmoothlone.restype = ctypes.c_double
        L.ref_sumsmoothlone.argtypes = [dp, ci, ctypes.c_double, ctypes.c_double]
        L.ref_sumsmoothlone_default_alpha.restype = ctypes.c_double
        L.ref_sumsmoothlone_default_alpha.argtypes = [dp, ci, ctypes.c_double]
        _LIBS[key] = L
    return _LIBS[key]


_f, _p, _ip, theta_table = _O._f, _O._p, _O._ip, _O.theta_table


class Reference:
    """The six exports, with oracle.py's signatures, on one loaded library."""

    def __init__(self, path: str | None = None):
        self.L = lib(path)

    def cov_rns(self, theta, locs, x_covariates, smooth_limits) -> np.ndarray:
        locs, X = _f(locs), _f(x_covariates)
        n, p = X.shape
        T = theta_table(theta)
        sl = np.asarray(smooth_limits, dtype=np.float64)
        out = np.empty((n, n), order="F")
        assert self.L.ref_cov_rns(n, p, _p(T), _p(locs), _p(X), _p(sl), _p(out)) == 0
        return out

    def cov_rns_classic(self, theta, locs, x_covariates) -> np.ndarray:
        locs, X = _f(locs), _f(x_covariates)
        n, p = X.shape
        T = theta_table(theta)
        out = np.empty((n, n), order="F")
        assert self.L.ref_cov_rns_classic(n, p, _p(T), _p(locs), _p(X), _p(out)) == 0
        return out

    def cov_rns_pred(self, theta, locs, locs_pred, x_covariates, x_covariates_pred, smooth_limits) -> np.ndarray:
        locs, lp, X, Xp = _f(locs), _f(locs_pred), _f(x_covariates), _f(x_covariates_pred)
        n, p = X.shape
        m = Xp.shape[0]
        T = theta_table(theta)
        sl = np.asarray(smooth_limits, dtype=np.float64)
        out = np.empty((m, n), order="F")
        assert self.L.ref_cov_rns_pred(n, m, p, _p(T), _p(locs), _p(lp), _p(X), _p(Xp), _p(sl), _p(out)) == 0
        return out

    def cov_rns_taper(self, theta, locs, x_covariates, colindices, rowpointers, smooth_limits) -> np.ndarray:
        locs, X = _f(locs), _f(x_covariates)
        n, p = X.shape
        T = theta_table(theta)
        sl = np.asarray(smooth_limits, dtype=np.float64)
        ci = np.ascontiguousarray(colindices, dtype=np.int32)
        rp = np.ascontiguousarray(rowpointers, dtype=np.int32)
        assert rp.size == n + 1 and rp[-1] - 1 == ci.size
        out = np.empty(ci.size)
        assert self.L.ref_cov_rns_taper(n, p, _p(T), _p(locs), _p(X), _p(sl), ci.size, _ip(ci), _ip(rp), _p(out)) == 0
        return out

    def cov_rns_taper_pred(self, theta, locs, locs_pred, x_covariates, x_covariates_pred, colindices, rowpointers,
                           smooth_limits) -> np.ndarray:
        locs, lp, X, Xp = _f(locs), _f(locs_pred), _f(x_covariates), _f(x_covariates_pred)
        n, p = X.shape
        m = Xp.shape[0]
        T = theta_table(theta)
        sl = np.asarray(smooth_limits, dtype=np.float64)
        ci = np.ascontiguousarray(colindices, dtype=np.int32)
        rp = np.ascontiguousarray(rowpointers, dtype=np.int32)
        assert rp.size == m + 1 and rp[-1] - 1 == ci.size
        out = np.empty(ci.size)
        assert self.L.ref_cov_rns_taper_pred(n, m, p, _p(T), _p(locs), _p(lp), _p(X), _p(Xp), _p(sl), ci.size,
                                             _ip(ci), _ip(rp), _p(out)) == 0
        return out

    def sumsmoothlone(self, x, lam: float, alpha: float | None = None) -> float:
        """alpha=None takes the reference's own default argument."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
        if alpha is None:
            return self.L.ref_sumsmoothlone_default_alpha(_p(x), x.size, float(lam))
        return self.L.ref_sumsmoothlone(_p(x), x.size, float(lam), float(alpha))
