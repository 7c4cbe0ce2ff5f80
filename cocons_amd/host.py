"""Host-side mirror of the reference's R interface for the dense hot path.

The reference's host language is R (absent from this image), so the host side
above the C ABI is written in Python with the reference's names, argument
meaning and error behaviour:

  cov_rns / cov_rns_classic / cov_rns_pred     R/RcppExports.R:21-46
  getModelLists / getScale                     R/getFunctions.R:570-616, :376-436
  sumsmoothlone / getPen (.cocons.getPen)      src/cocons_full.cpp:12-30, R/checkFunctions.R:474-492
  GetNeg2loglikelihood[Profile|REML]           R/neg2loglikelihood.R:183-222, :127-165, :241-291
  cocoPredict_dense                            R/predict.R:136-187 (dense branch)

All heavy arithmetic runs in the HIP library; this module only does the O(p)
theta plumbing the reference also keeps on the host.  There is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import CholeskyError, c_dp


class KrigeJointNotPositiveDefinite(_lib.CoconsHipError):
    """cocons_krige_joint's and cocons_krige_taper_joint's -5: the predictive covariance is not positive definite in floating
    point (the message names the failing minor); the reference's second `chol` fails there (R/sim.R:106)."""


ASPECTS = ("mean", "std.dev", "scale", "aniso", "tilt", "smooth", "nugget")   # R/profile.R:5-7
COV_ASPECTS = ASPECTS[1:]


def _f(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _p(a):
    return a.ctypes.data_as(c_dp)


def theta_table(theta) -> np.ndarray:
    """Named list of length-p vectors -> the 6 x p row-major table of the C ABI.
    Looked up by name like src/cocons_full.cpp:47-54, so `theta_list` and
    `theta_list[-1]` both work."""
    rows = [np.asarray(theta[k], dtype=np.float64).ravel() for k in COV_ASPECTS]
    p = rows[0].size
    if any(r.size != p for r in rows):
        raise ValueError("theta aspects must have equal length")
    if p > _lib.P_MAX:
        raise ValueError("design matrix has %d columns; the HIP path supports up to %d" % (p, _lib.P_MAX))
    return np.ascontiguousarray(np.stack(rows, axis=0))


def _table_mean(theta):
    """(`theta_table`, the mean vector) of a named list: what the entries with a mean take"""
    return theta_table(theta), np.ascontiguousarray(np.asarray(theta["mean"], dtype=np.float64))


# --------------------------------------------------------------------------- #
# covariance assembly (.Call surface)
# --------------------------------------------------------------------------- #
def cov_rns(theta, locs, x_covariates, smooth_limits) -> np.ndarray:
    """Dense covariance function (difference parameterization); R/RcppExports.R:21-23."""
    L = _lib.load()
    locs, X = _f(locs), _f(x_covariates)
    n, p = X.shape
    T = theta_table(theta)
    sl = np.asarray(smooth_limits, dtype=np.float64)
    out = np.empty((n, n), order="F")
    _lib.check(L.cocons_cov_rns(n, p, _p(T), _p(locs), _p(X), _p(sl), _p(out)), "cov_rns")
    return out


def cov_rns_classic(theta, locs, x_covariates) -> np.ndarray:
    """Dense covariance function (classic parameterization); R/RcppExports.R:44-46."""
    L = _lib.load()
    locs, X = _f(locs), _f(x_covariates)
    n, p = X.shape
    T = theta_table(theta)
    out = np.empty((n, n), order="F")
    _lib.check(L.cocons_cov_rns_classic(n, p, _p(T), _p(locs), _p(X), _p(out)), "cov_rns_classic")
    return out


def cov_rns_pred(theta, locs, locs_pred, x_covariates, x_covariates_pred, smooth_limits) -> np.ndarray:
    """Cross-covariance, m x n with row = prediction location; R/RcppExports.R:34-36."""
    L = _lib.load()
    locs, lp, X, Xp = _f(locs), _f(locs_pred), _f(x_covariates), _f(x_covariates_pred)
    n, p = X.shape
    m = Xp.shape[0]
    T = theta_table(theta)
    sl = np.asarray(smooth_limits, dtype=np.float64)
    out = np.empty((m, n), order="F")
    _lib.check(L.cocons_cov_rns_pred(n, m, p, _p(T), _p(locs), _p(lp), _p(X), _p(Xp), _p(sl), _p(out)),
               "cov_rns_pred")
    return out


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _csr(taper):
    """(colindices int32, rowpointers int32, entries float64), contiguous, of a (colindices, rowpointers, entries) triple"""
    return (np.ascontiguousarray(np.asarray(taper[0], dtype=np.int32)), np.ascontiguousarray(np.asarray(taper[1], dtype=np.int32)),
            np.ascontiguousarray(np.asarray(taper[2], dtype=np.float64)))


def cov_rns_taper(theta, locs, x_covariates, colindices, rowpointers, smooth_limits) -> np.ndarray:
    """Sparse covariance function: the entries of the spam pattern (colindices / rowpointers 1-based, as
    spam stores them); R/RcppExports.R:63-65 -> src/cocons_taper.cpp:151-433."""
    L = _lib.load()
    locs, X = _f(locs), _f(x_covariates)
    n, p = X.shape
    T = theta_table(theta)
    sl = np.asarray(smooth_limits, dtype=np.float64)
    ci = np.ascontiguousarray(colindices, dtype=np.int32)
    rp = np.ascontiguousarray(rowpointers, dtype=np.int32)
    out = np.empty(ci.size)
    _lib.check(L.cocons_cov_rns_taper(n, p, _p(T), _p(locs), _p(X), _p(sl), ci.size, _ip(ci), _ip(rp), _p(out)),
               "cov_rns_taper")
    return out


def cov_rns_taper_pred(theta, locs, locs_pred, x_covariates, x_covariates_pred, colindices, rowpointers,
                       smooth_limits) -> np.ndarray:
    """Sparse cross-covariance entries (rows = prediction locations); R/RcppExports.R:52-54 ->
    src/cocons_taper.cpp:17-139."""
    L = _lib.load()
    locs, lp, X, Xp = _f(locs), _f(locs_pred), _f(x_covariates), _f(x_covariates_pred)
    n, p = X.shape
    m = Xp.shape[0]
    T = theta_table(theta)
    sl = np.asarray(smooth_limits, dtype=np.float64)
    ci = np.ascontiguousarray(colindices, dtype=np.int32)
    rp = np.ascontiguousarray(rowpointers, dtype=np.int32)
    out = np.empty(ci.size)
    _lib.check(L.cocons_cov_rns_taper_pred(n, m, p, _p(T), _p(locs), _p(lp), _p(X), _p(Xp), _p(sl), ci.size,
                                           _ip(ci), _ip(rp), _p(out)), "cov_rns_taper_pred")
    return out


def sumsmoothlone(x, lam: float, alpha: float = 1e6) -> float:
    """Smoothed-L1 penalty; R/RcppExports.R:10-12 (host arithmetic, O(p))."""
    L = _lib.load()
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    return L.cocons_sumsmoothlone(_p(x), x.size, float(lam), float(alpha))


# --------------------------------------------------------------------------- #
# theta plumbing -- stays on the host in the reference too
# --------------------------------------------------------------------------- #
def _is_logical(v) -> bool:
    return isinstance(v, (list, tuple, np.ndarray)) and len(v) > 0 and \
        all(isinstance(b, (bool, np.bool_)) for b in v)


def getModelLists(theta, par_pos, type="diff"):
    """R/getFunctions.R:570-616."""
    theta = np.asarray(theta, dtype=np.float64).ravel()
    length_logical = max(len(v) if _is_logical(v) else 1 for v in par_pos.values())
    out = OrderedDict()
    acum = 0
    for name, pp in par_pos.items():
        vec = np.zeros(length_logical)
        if not _is_logical(pp):
            vec[0] = float(np.asarray(pp, dtype=np.float64).ravel()[0])
        else:
            mask = np.asarray(pp, dtype=bool)
            k = int(mask.sum())
            full = np.zeros(len(mask))
            full[mask] = theta[acum:acum + k]
            vec[:len(mask)] = full
            acum += k
        out[name] = vec
    if type == "classic":
        return out
    if type != "diff":
        raise ValueError("type must be 'diff' or 'classic'")
    sd_pp, sc_pp = par_pos["std.dev"], par_pos["scale"]
    if _is_logical(sd_pp) and _is_logical(sc_pp):
        tmp = OrderedDict((k, v.copy()) for k, v in out.items())
        for i in range(len(sd_pp)):
            if sd_pp[i] and sc_pp[i]:
                tmp["std.dev"][i] = (out["std.dev"][i] + out["scale"][i]) / 2
                tmp["scale"][i] = (out["std.dev"][i] - out["scale"][i]) / 2
        return tmp
    return out


def getScale(x, mean_vector=None, sd_vector=None):
    """R/getFunctions.R:410-434 (matrix branch)."""
    x = np.array(x, dtype=np.float64, copy=True, order="F")
    if mean_vector is None:
        mean_vector = x.mean(axis=0)
        mean_vector[0] = 0.0
    if sd_vector is None:
        sd_vector = x.std(axis=0, ddof=1) if x.shape[0] > 1 else np.ones(x.shape[1])
        sd_vector[0] = 1.0
    for ii in range(1, x.shape[1]):
        x[:, ii] = (x[:, ii] - mean_vector[ii]) / sd_vector[ii]
    return {"std.covs": x, "mean.vector": np.asarray(mean_vector), "sd.vector": np.asarray(sd_vector)}


def getPen(n, lam, theta_list, smooth_limits) -> float:
    """.cocons.getPen; R/checkFunctions.R:474-492 (lambda = Sigma, betas, reg)."""
    names = list(theta_list.keys())
    summ = lam[2] * math.exp(theta_list["scale"][0]) * math.sqrt(
        (smooth_limits[1] - smooth_limits[0]) / (1 + math.exp(-theta_list["smooth"][0])) + smooth_limits[0]
    ) + sumsmoothlone(theta_list[names[0]][1:], lam[1])
    for ii in range(1, 6):
        summ += sumsmoothlone(theta_list[names[ii]][1:], lam[0])
    return 2 * n * summ


def _dsumsmoothlone(x, lam: float, alpha: float = 1e6) -> np.ndarray:
    """Derivative of `sumsmoothlone` per element: sign(x) where |x| > 1e-4, tanh(alpha x / 2) on the smooth branch."""
    x = np.asarray(x, dtype=np.float64).ravel()
    return lam * np.where(np.abs(x) > 1e-4, np.sign(x), np.tanh(alpha * x / 2))


def getPen_grad(n, lam, theta_list, smooth_limits) -> OrderedDict:
    """Exact derivative of `getPen` with respect to every entry of theta_list (same keys, same shapes)."""
    names = list(theta_list.keys())
    g = OrderedDict((k, np.zeros(np.asarray(v, dtype=np.float64).size)) for k, v in theta_list.items())
    lo, hi = smooth_limits[0], smooth_limits[1]
    sc0, sm0 = float(theta_list["scale"][0]), float(theta_list["smooth"][0])
    s = 1 / (1 + math.exp(-sm0))
    nu0 = (hi - lo) * s + lo
    g["scale"][0] += lam[2] * math.exp(sc0) * math.sqrt(nu0)
    g["smooth"][0] += lam[2] * math.exp(sc0) * (hi - lo) * s * (1 - s) / (2 * math.sqrt(nu0))
    g[names[0]][1:] += _dsumsmoothlone(theta_list[names[0]][1:], lam[1])
    for ii in range(1, 6):
        g[names[ii]][1:] += _dsumsmoothlone(theta_list[names[ii]][1:], lam[0])
    for k in g:
        g[k] *= 2 * n
    return g


def getModelLists_grad(grad_lists, par_pos) -> np.ndarray:
    """Chain rule through getModelLists(type="diff"): the gradient over the table entries (named lists) -> the gradient over
    the optimiser's vector.  Where std.dev and scale are both free, d/d raw_sd = (g_sd + g_sc) / 2 and
    d/d raw_sc = (g_sd - g_sc) / 2."""
    g = OrderedDict((k, np.asarray(v, dtype=np.float64).ravel().copy()) for k, v in grad_lists.items())
    sd_pp, sc_pp = par_pos["std.dev"], par_pos["scale"]
    if _is_logical(sd_pp) and _is_logical(sc_pp):
        gsd, gsc = g["std.dev"].copy(), g["scale"].copy()
        for i in range(len(sd_pp)):
            if sd_pp[i] and sc_pp[i]:
                g["std.dev"][i] = (gsd[i] + gsc[i]) / 2
                g["scale"][i] = (gsd[i] - gsc[i]) / 2
    out = []
    for name, pp in par_pos.items():
        if _is_logical(pp):
            out.extend(g[name][:len(pp)][np.asarray(pp, dtype=bool)].tolist())
    return np.asarray(out)


# --------------------------------------------------------------------------- #
# fit handle: data that is constant over an optimisation stays in HBM
# --------------------------------------------------------------------------- #
class _Handle:
    """What the dense, the tapered and the Vecchia handle share: the data of the fit taken onto the object, and its end."""

    def _adopt(self, locs, x_covariates, z, smooth_limits):
        """Loads the library and sets n, p, r, q = 0, smooth_limits and x_covariates; returns (locs, X, z) as the create
        entries take them."""
        self._L = _lib.load()
        locs, X = _f(locs), _f(x_covariates)
        self.n, self.p = X.shape
        if locs.shape != (self.n, 2):
            raise ValueError("locs must be n x 2")
        z = _f(np.asarray(z, dtype=np.float64).reshape(self.n, -1))
        self.r = z.shape[1]
        self.q = 0
        self.smooth_limits = np.asarray(smooth_limits, dtype=np.float64).copy()
        self.x_covariates = X
        return locs, X, z

    def _created(self, h, entry):
        self._h = h
        if not h:
            raise _lib.CoconsHipError(entry + " failed: " + _lib.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._L.cocons_fit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextlib.contextmanager
def _borrowed(fit, make):
    """The caller's handle `fit`, or make() for the length of the block, closed on the way out."""
    if fit is not None:
        yield fit
        return
    f = make()
    try:
        yield f
    finally:
        f.close()


def _dense(fit, locs, x_covariates, z, smooth_limits, x_betas=None):
    return _borrowed(fit, lambda: CoconsFit(locs, x_covariates, z, smooth_limits, x_betas=x_betas))


def _tapered(fit, locs, x_covariates, z, smooth_limits, ref_taper):
    return _borrowed(fit, lambda: CoconsTaperFit(locs, x_covariates, z, smooth_limits, *ref_taper))


def _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped=False):
    make = CoconsVecchiaFit.from_groups if grouped else CoconsVecchiaFit
    return _borrowed(fit, lambda: make(locs, x_covariates, z, smooth_limits, nn))


@contextlib.contextmanager
def _held(prepare, release, *args, **kwargs):
    """A held factor for the length of the block: prepare(*args, **kwargs), and release on the way out."""
    prepare(*args, **kwargs)
    try:
        yield
    finally:
        release()


@contextlib.contextmanager
def _chol_error(*also):
    """Outside the objectives a failing `chol` propagates in the reference (base::chol, spam::chol): CholeskyError, and
    the exceptions of `also`, become its RuntimeError."""
    try:
        yield
    except (CholeskyError,) + also:
        raise RuntimeError("Cholesky error")


def _fold_labels(fold, n):
    """(nfold, the n labels in [0, nfold) as int32) of a cv_core's `fold`"""
    lab = np.ascontiguousarray(np.asarray(fold).ravel(), dtype=np.int32)
    if lab.size != n:
        raise ValueError("fold must have length n")
    return (int(lab.max()) + 1 if lab.size and lab.max() >= 0 else 1), lab


def _check_joint(rc, entry):
    """`_lib.check` for the two joint entries, whose -5 is also a predictive covariance that is not positive definite
    (and a hand-off time-out that was repeated in vain: told apart by the message)"""
    if rc == -5 and "not positive definite" in _lib.last_error():
        raise KrigeJointNotPositiveDefinite(_lib.last_error())
    _lib.check(rc, entry)


class CoconsFit(_Handle):
    """Device-resident (locs, x_covariates, z [, x_betas], smooth.limits) of one fit --
    the arguments the reference passes unchanged to every objective evaluation
    (R/optim.R:237-259).  Only O(p) bytes cross PCIe per evaluation."""

    def __init__(self, locs, x_covariates, z, smooth_limits, x_betas=None, device=-1):
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        xb = None
        if x_betas is not None:
            xb = _f(np.asarray(x_betas, dtype=np.float64).reshape(self.n, -1))
            self.q = xb.shape[1]
        self._created(self._L.cocons_fit_create(self.n, self.p, self.r, self.q, _p(locs), _p(X), _p(z),
                                                _p(xb) if xb is not None else None, _p(self.smooth_limits), int(device)),
                      "cocons_fit_create")

    # -- cores (no penalty) ---------------------------------------------------
    def neg2loglik_core(self, theta_list):
        T, mean = _table_mean(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(1 + self.r)
        _lib.check(self._L.cocons_neg2loglik_dense(self._h, _p(T), _p(mean), ctypes.byref(val), _p(parts)),
                   "cocons_neg2loglik_dense")
        return val.value, parts

    def neg2loglik_grad_core(self, theta_list):
        """The value of `neg2loglik_core` and its analytic gradient (cocons_neg2loglik_grad_dense): returns
        (value, parts, grad_table 6 x p in the order std.dev, scale, aniso, tilt, smooth, nugget, grad_mean p)."""
        T, mean = _table_mean(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(1 + self.r)
        gt = np.zeros((6, self.p))
        gm = np.zeros(self.p)
        _lib.check(self._L.cocons_neg2loglik_grad_dense(self._h, _p(T), _p(mean), ctypes.byref(val), _p(parts), _p(gt),
                                                         _p(gm)),
                   "cocons_neg2loglik_grad_dense")
        return val.value, parts, gt, gm

    def fisher_core(self, theta_list, dirs):
        """Expected information of the dense model at `theta_list` (cocons_fisher_dense).  `dirs`: ndir directions in
        table space, ndir x 6 x p (or ndir x 6p) in the order std.dev, scale, aniso, tilt, smooth, nugget.  Returns
        (info ndir x ndir = (r / 2) tr(Sigma^-1 Sigma_a Sigma^-1 Sigma_b), info_mean p x p = r X' Sigma^-1 X)."""
        T = theta_table(theta_list)
        D = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 6 * self.p))
        nd = D.shape[0]
        info = np.zeros((nd, nd))
        info_mean = np.zeros((self.p, self.p))
        _lib.check(self._L.cocons_fisher_dense(self._h, _p(T), nd, _p(D), _p(info), _p(info_mean)), "cocons_fisher_dense")
        return info, info_mean

    def fisher_reml_core(self, theta_list, dirs):
        """Expected information of the REML fit at `theta_list` (cocons_fisher_reml), `dirs` as for `fisher_core`:
        info ndir x ndir = (r / 2) tr(P Sigma_a P Sigma_b), P = Sigma^-1 - Sigma^-1 X (X' Sigma^-1 X)^-1 X' Sigma^-1.
        There is no mean block."""
        T = theta_table(theta_list)
        D = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 6 * self.p))
        nd = D.shape[0]
        info = np.zeros((nd, nd))
        _lib.check(self._L.cocons_fisher_reml(self._h, _p(T), nd, _p(D), _p(info)), "cocons_fisher_reml")
        return info

    def cv_core(self, theta_list, fold=None):
        """Cross-validated predictions from one factorisation (cocons_cv_dense).  `fold`: n integer labels in [0, nfold)
        (None: leave-one-out).  Returns (resid n x r = z minus its prediction from the observations outside the fold,
        var n = the predictive variance, nugget included)."""
        T, mean = _table_mean(theta_list)
        resid = np.zeros((self.n, self.r), order="F")
        var = np.zeros(self.n)
        nfold, lab = (0, None) if fold is None else _fold_labels(fold, self.n)
        _lib.check(self._L.cocons_cv_dense(self._h, _p(T), _p(mean), nfold, None if lab is None else _ip(lab), _p(resid),
                                           _p(var)), "cocons_cv_dense")
        return resid, var

    def neg2loglik_batch_core(self, theta_lists):
        """Independent evaluations pipelined on the GPU (cocons_neg2loglik_batch).  Returns
        (values, status) arrays; status k > 0 marks a Cholesky failure at minor k."""
        nb = len(theta_lists)
        T = np.ascontiguousarray(np.stack([theta_table(t) for t in theta_lists], axis=0)) if nb else np.zeros((0, 6, self.p))
        M = np.ascontiguousarray(np.stack([np.asarray(t["mean"], dtype=np.float64) for t in theta_lists], axis=0)) \
            if nb else np.zeros((0, self.p))
        vals = np.zeros(nb)
        st = np.zeros(nb, dtype=np.int32)
        _lib.check(self._L.cocons_neg2loglik_batch(self._h, nb, _p(T), _p(M), _p(vals),
                                                   st.ctypes.data_as(ctypes.POINTER(ctypes.c_int))),
                   "cocons_neg2loglik_batch")
        return vals, st

    def neg2loglik_profile_core(self, theta_list):
        T = theta_table(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(2 + self.r + self.q)
        _lib.check(self._L.cocons_neg2loglik_profile(self._h, _p(T), ctypes.byref(val), _p(parts)),
                   "cocons_neg2loglik_profile")
        return val.value, parts

    def neg2loglik_reml_core(self, theta_list, rank):
        T = theta_table(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(2 + self.r + self.p)
        _lib.check(self._L.cocons_neg2loglik_reml(self._h, _p(T), int(rank), ctypes.byref(val), _p(parts)),
                   "cocons_neg2loglik_reml")
        return val.value, parts

    def neg2loglik_profile_grad_core(self, theta_list):
        """The value and parts of `neg2loglik_profile_core` and the analytic gradient over the 6 x p table
        (cocons_neg2loglik_profile_grad): (value, parts, grad_table).  The mean is profiled out: no mean gradient."""
        T = theta_table(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(2 + self.r + self.q)
        gt = np.zeros((6, self.p))
        _lib.check(self._L.cocons_neg2loglik_profile_grad(self._h, _p(T), ctypes.byref(val), _p(parts), _p(gt)),
                   "cocons_neg2loglik_profile_grad")
        return val.value, parts, gt

    def neg2loglik_reml_grad_core(self, theta_list, rank):
        """The same for `neg2loglik_reml_core` (cocons_neg2loglik_reml_grad)."""
        T = theta_table(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(2 + self.r + self.p)
        gt = np.zeros((6, self.p))
        _lib.check(self._L.cocons_neg2loglik_reml_grad(self._h, _p(T), int(rank), ctypes.byref(val), _p(parts), _p(gt)),
                   "cocons_neg2loglik_reml_grad")
        return val.value, parts, gt

    def predict_core(self, theta_list, locs_pred, x_covariates_pred, z_col=0):
        T, mean = _table_mean(theta_list)
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        m = Xp.shape[0]
        st, qf = np.zeros(m), np.zeros(m)
        _lib.check(self._L.cocons_predict_dense(self._h, _p(T), _p(mean), int(z_col), m, _p(lp), _p(Xp),
                                                _p(st), _p(qf)), "cocons_predict_dense")
        return st, qf

    def krige_prepare(self, theta_list, z_col=0, max_rows=0):
        """Factor Sigma(theta) once and keep the factor on the handle (cocons_krige_prepare): krige_core then predicts
        at any number of new locations without factoring again.  max_rows: rows per chunk (0: the library's default)."""
        T, mean = _table_mean(theta_list)
        _lib.check(self._L.cocons_krige_prepare(self._h, _p(T), _p(mean), int(z_col), int(max_rows)),
                   "cocons_krige_prepare")

    def krige_core(self, locs_pred, x_covariates_pred):
        """(stochastic, quadform) at the new locations against the prepared factor, as predict_core gives them."""
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        m = Xp.shape[0]
        st, qf = np.empty(m), np.empty(m)
        _lib.check(self._L.cocons_krige_apply(self._h, m, _p(lp), _p(Xp), _p(st), _p(qf)), "cocons_krige_apply")
        return st, qf

    def krige_joint_core(self, locs_pred, x_covariates_pred, locs_unobs=None, iiderrors=None, cov=True):
        """(stochastic, cov | None, sims | None) at the new locations against the prepared factor (cocons_krige_joint):
        cov = Sigma_uu - C Sigma^-1 C' (m x m, symmetric to the bit; Sigma_uu at locs_unobs, default locs_pred), sims =
        chol(cov) iiderrors + (X_pred mean + stochastic) for iiderrors m x nsim.  A predictive covariance that is not
        positive definite in floating point (draws only) raises KrigeJointNotPositiveDefinite; nothing is returned then."""
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        m = Xp.shape[0]
        lu = None if locs_unobs is None else _f(np.asarray(locs_unobs, dtype=np.float64)[:, :2])
        E = None if iiderrors is None else _f(np.asarray(iiderrors, dtype=np.float64).reshape(m, -1))
        nsim = 0 if E is None else E.shape[1]
        st = np.empty(m)
        C = np.empty((m, m), order="F") if cov else None
        Y = np.empty((m, nsim), order="F") if nsim > 0 else None
        rc = self._L.cocons_krige_joint(self._h, m, _p(lp), _p(Xp), None if lu is None else _p(lu), _p(st),
                                        None if C is None else _p(C), nsim, None if nsim == 0 else _p(E),
                                        None if Y is None else _p(Y))
        _check_joint(rc, "cocons_krige_joint")
        return st, C, Y

    def krige_release(self):
        _lib.check(self._L.cocons_krige_release(self._h), "cocons_krige_release")

    def krige_held(self, theta_list, z_col=0, max_rows=0):
        """`with fit.krige_held(theta_list):` -- krige_prepare on the way in, krige_release on the way out"""
        return _held(self.krige_prepare, self.krige_release, theta_list, z_col, max_rows)

    def krige_info(self):
        """{prepared, bytes, rows, n}: whether a state is held, its device bytes, rows per chunk, observations."""
        out = (ctypes.c_longlong * 4)()
        _lib.check(self._L.cocons_krige_info(self._h, out), "cocons_krige_info")
        return {"prepared": bool(out[0]), "bytes": int(out[1]), "rows": int(out[2]), "n": int(out[3])}

    def cov_rows(self, theta_list, index, cor=False, classic=False):
        """Rows `index` (0-based) of cov_rns / cov_rns_classic at the fit's locations, or of cov2cor of it,
        without the n x n matrix (what plot(type = "correlations") reads, R/methods.R:161-165)."""
        T = theta_table(theta_list)
        idx = np.ascontiguousarray(np.atleast_1d(index), dtype=np.int32)
        out = np.empty((idx.size, self.n))
        _lib.check(self._L.cocons_cov_rows(self._h, _p(T), int(bool(classic)), idx.size, _ip(idx), int(bool(cor)), _p(out)),
                   "cocons_cov_rows")
        return out

    def sim_core(self, theta_list, iiderrors, classic=False):
        E = _f(np.asarray(iiderrors, dtype=np.float64).reshape(self.n, -1))
        T, mean = _table_mean(theta_list)
        out = np.empty(E.shape, order="F")
        _lib.check(self._L.cocons_sim_dense(self._h, _p(T), _p(mean), 1 if classic else 0, E.shape[1], _p(E), _p(out)),
                   "cocons_sim_dense")
        return out

    def sim_cond_core(self, theta_list, locs_pred, x_covariates_pred, locs_unobs, iiderrors, z_col=0):
        lp, Xp, lu = _f(locs_pred), _f(x_covariates_pred), _f(np.asarray(locs_unobs, dtype=np.float64)[:, :2])
        m = Xp.shape[0]
        E = _f(np.asarray(iiderrors, dtype=np.float64).reshape(m, -1))
        T, mean = _table_mean(theta_list)
        out = np.empty(E.shape, order="F")
        _lib.check(self._L.cocons_sim_cond_dense(self._h, _p(T), _p(mean), int(z_col), m, _p(lp), _p(Xp), _p(lu),
                                                 E.shape[1], _p(E), _p(out)), "cocons_sim_cond_dense")
        return out

    def engine_state(self):
        """{"active": last completed operation ran on the engine schedule, "retries": hand-off time-outs so far (each
        repeated once on the plain schedule), "last_abort": code of the last one} -- cocons_fit_engine_state."""
        out = (ctypes.c_int * 3)()
        _lib.check(self._L.cocons_fit_engine_state(self._h, out), "cocons_fit_engine_state")
        return {"active": bool(out[0]), "retries": int(out[1]), "last_abort": int(out[2])}

    def stream(self):
        """The hipStream_t the handle launches on, as an integer (0: the NULL stream) -- cocons_fit_stream."""
        return int(self._L.cocons_fit_stream(self._h) or 0)

    def set_stream(self, stream):
        """Launch on the caller's stream from now on (a hipStream_t as an integer, e.g. torch.cuda.Stream().cuda_stream;
        None or 0: the NULL stream) -- cocons_fit_set_stream."""
        _lib.check(self._L.cocons_fit_set_stream(self._h, ctypes.c_void_p(int(stream or 0) or None)), "cocons_fit_set_stream")

    def sync(self):
        """Wait for everything the handle has enqueued on its stream -- cocons_fit_sync."""
        _lib.check(self._L.cocons_fit_sync(self._h), "cocons_fit_sync")

    def profile_stages(self, theta_list, reps=3):
        """Stage timings (ms) from HIP events on the fit's stream; see cocons_fit_profile."""
        T, mean = _table_mean(theta_list)
        ms = np.zeros(10)
        _lib.check(self._L.cocons_fit_profile(self._h, _p(T), _p(mean), int(reps), _p(ms)), "cocons_fit_profile")
        return {"assembly_ms": ms[0], "cholesky_ms": ms[1], "reduce_ms": ms[2], "eval_ms": ms[3],
                "update_avg_ms": ms[4], "update_launches": int(ms[5]), "update_sum_ms": ms[6],
                "update_flops": ms[7], "dag_ms": ms[8], "dag_flops": ms[9]}


TAPER_KINDS = {"wend1": 1, "wend2": 2, "sph": 3}


def _taper_kind(kind) -> int:
    if isinstance(kind, str):
        if kind not in TAPER_KINDS:
            raise ValueError("kind must be one of %s" % sorted(TAPER_KINDS))
        return TAPER_KINDS[kind]
    return int(kind)


def taper_pattern(locs, delta, kind="wend1", newlocs=None, device=0):
    """(colindices, rowpointers, entries) of the taper between `newlocs` (default: locs themselves) and locs, found on the
    device (cocons_taper_pattern): spam's nearest.dist(newlocs, locs, delta) -- every pair with d <= delta, zero distances
    and the diagonal stored, 1-based CSR with ascending columns -- with cov.wend1 / cov.wend2 / cov.sph at
    theta = c(delta, 1) as entries.  One count call, then the fill call."""
    L = _lib.load()
    locs = _f(locs)
    n = locs.shape[0]
    q = None if newlocs is None else _f(newlocs)
    m = n if q is None else q.shape[0]
    k = _taper_kind(kind)
    nnz = ctypes.c_longlong(0)
    rp = np.zeros(m + 1, dtype=np.int32)
    qp = None if q is None else _p(q)
    _lib.check(L.cocons_taper_pattern(n, _p(locs), m, qp, float(delta), k, int(device), 0, ctypes.byref(nnz), _ip(rp), None,
                                      None), "cocons_taper_pattern")
    ci = np.zeros(max(int(nnz.value), 1), dtype=np.int32)
    ent = np.zeros(max(int(nnz.value), 1))
    _lib.check(L.cocons_taper_pattern(n, _p(locs), m, qp, float(delta), k, int(device), int(nnz.value), ctypes.byref(nnz),
                                      _ip(rp), _ip(ci), _p(ent)), "cocons_taper_pattern")
    return ci[:nnz.value], rp, ent[:nnz.value]


class CoconsTaperFit(CoconsFit):
    """Handle of an optimisation of GetNeg2loglikelihoodTaper: (locs, x_covariates, z, smooth.limits) plus the
    spam pattern of `ref_taper` (colindices / rowpointers, 1-based, symmetric, diagonal stored) and its entries.
    `neg2loglik_core` (inherited) then evaluates the -2 log-likelihood core of the TAPERED covariance through the
    dense factorisation -- spam's value while n^2 doubles fit the device.  Everything else a dense handle
    offers is refused by the library."""

    def __init__(self, locs, x_covariates, z, smooth_limits, colindices, rowpointers, taper_entries, device=-1):
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        ci, rp, te = _csr((colindices, rowpointers, taper_entries))
        if te.size != ci.size:
            raise ValueError("taper entries and colindices differ in length")
        self._created(self._L.cocons_fit_create_taper(self.n, self.p, self.r, _p(locs), _p(X), _p(z), _p(self.smooth_limits),
                                                      int(device), int(ci.size), _ip(ci), _ip(rp), _p(te)),
                      "cocons_fit_create_taper")

    @classmethod
    def from_delta(cls, locs, x_covariates, z, smooth_limits, delta, kind="wend1", device=-1):
        """The handle of the taper `kind` with range `delta`: the library finds the pattern and its entries itself
        (cocons_fit_create_taper_delta), then builds what __init__ builds from them."""
        self = cls.__new__(cls)
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        self._created(self._L.cocons_fit_create_taper_delta(self.n, self.p, self.r, _p(locs), _p(X), _p(z),
                                                            _p(self.smooth_limits), int(device), float(delta),
                                                            _taper_kind(kind)), "cocons_fit_create_taper_delta")
        return self

    def neg2loglik_grad_core(self, theta_list):
        """The value of `neg2loglik_core` on this handle and its analytic gradient (cocons_neg2loglik_grad_taper): returns
        (value, parts, grad_table, grad_quad, grad_mean) -- the 6 x p table of the whole value in the order std.dev, scale,
        aniso, tilt, smooth, nugget (aniso and tilt rows zero), the same table for the quadratic forms alone (the
        log-determinant's part is grad_table - grad_quad), and the mean gradient."""
        T, mean = _table_mean(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(1 + self.r)
        gt = np.zeros((6, self.p))
        gq = np.zeros((6, self.p))
        gm = np.zeros(self.p)
        _lib.check(self._L.cocons_neg2loglik_grad_taper(self._h, _p(T), _p(mean), ctypes.byref(val), _p(parts), _p(gt),
                                                         _p(gq), _p(gm)),
                   "cocons_neg2loglik_grad_taper")
        return val.value, parts, gt, gq, gm

    def fisher_core(self, theta_list, dirs, probes=None, max_rows=0):
        """Expected information of the tapered model at `theta_list` on the band factor (cocons_fisher_taper).  `dirs` as
        for `CoconsFit.fisher_core` (ndir x 6 x p), under the taper gradient's conventions (full scale vector; the aniso
        and tilt rows do not enter).  probes = None: the n unit vectors, exact, O(ndir n^2 bandwidth); else an n x nprobe
        array whose columns are probes in the caller's observation order with E[e e'] = I (Hutchinson's estimator).
        max_rows: probe rows per chunk (0: the library's default); the result does not depend on it.  Returns
        (info ndir x ndir = (r / 2) tr(S^-1 S_a S^-1 S_b), info_mean p x p = r X' S^-1 X, exact in both modes)."""
        T = theta_table(theta_list)
        D = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 6 * self.p))
        nd = D.shape[0]
        info = np.zeros((nd, nd))
        info_mean = np.zeros((self.p, self.p))
        if probes is None:
            npr, P = 0, None
        else:
            P = _f(np.asarray(probes, dtype=np.float64).reshape(self.n, -1))
            npr = P.shape[1]
        _lib.check(self._L.cocons_fisher_taper(self._h, _p(T), nd, _p(D), int(npr), None if P is None else _p(P),
                                               int(max_rows), _p(info), _p(info_mean)), "cocons_fisher_taper")
        return info, info_mean

    def cv_core(self, theta_list, fold=None, max_rows=0):
        """Cross-validated predictions of the tapered model: (resid n x r, var n) as `CoconsFit.cv_core` gives them.
        `fold` = None: leave-one-out from the selected inverse (cocons_cv_taper).  `fold`: n integer labels in [0, nfold) --
        every fold from the one held band factor (cocons_cv_taper_folds), in chunks of `max_rows` rows of the band solve
        (0: the library's choice); `last_cv_stats` then holds the call's five counts (folds of one observation, of 2 .. 128,
        larger, chunks run, device bytes of the call)."""
        T, mean = _table_mean(theta_list)
        resid = np.zeros((self.n, self.r), order="F")
        var = np.zeros(self.n)
        if fold is None:
            _lib.check(self._L.cocons_cv_taper(self._h, _p(T), _p(mean), _p(resid), _p(var)), "cocons_cv_taper")
            return resid, var
        nfold, lab = _fold_labels(fold, self.n)
        stats = (ctypes.c_longlong * 5)()
        _lib.check(self._L.cocons_cv_taper_folds(self._h, _p(T), _p(mean), nfold, _ip(lab), int(max_rows), _p(resid), _p(var),
                                                 stats), "cocons_cv_taper_folds")
        self.last_cv_stats = [int(v) for v in stats]
        return resid, var

    def predict_core(self, theta_list, locs_pred, x_covariates_pred, pred_taper, z_col=0):
        """(stochastic, quadform) of the sparse branch of cocoPredict; pred_taper = (colindices, rowpointers,
        entries) of the m x n taper between prediction and observed locations (1-based CSR)."""
        T, mean = _table_mean(theta_list)
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        m = Xp.shape[0]
        ci, rp, te = _csr(pred_taper)
        st, qf = np.empty(m), np.empty(m)
        _lib.check(self._L.cocons_predict_taper(self._h, _p(T), _p(mean), int(z_col), m, _p(lp), _p(Xp), int(ci.size),
                                                _ip(ci), _ip(rp), _p(te), _p(st), _p(qf)), "cocons_predict_taper")
        return st, qf

    def krige_taper_prepare(self, theta_list, z_col=0, max_rows=0):
        """Factor the tapered S(theta) once and keep the band factor on the handle (cocons_krige_taper_prepare):
        krige_taper_core then predicts at any number of new locations without factoring again.  max_rows: rows per
        chunk (0: the library's default)."""
        T, mean = _table_mean(theta_list)
        _lib.check(self._L.cocons_krige_taper_prepare(self._h, _p(T), _p(mean), int(z_col), int(max_rows)),
                   "cocons_krige_taper_prepare")

    def krige_taper_core(self, locs_pred, x_covariates_pred, pred_taper):
        """(stochastic, quadform) at the new locations against the prepared band factor, as predict_core gives them;
        pred_taper as predict_core takes it, its columns strictly increasing within a row."""
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        m = Xp.shape[0]
        ci, rp, te = _csr(pred_taper)
        st, qf = np.empty(m), np.empty(m)
        _lib.check(self._L.cocons_krige_taper_apply(self._h, m, _p(lp), _p(Xp), int(ci.size), _ip(ci), _ip(rp), _p(te),
                                                    _p(st), _p(qf)), "cocons_krige_taper_apply")
        return st, qf

    def krige_taper_core_delta(self, locs_pred, x_covariates_pred, delta, kind="wend1"):
        """krige_taper_core without a pattern: the neighbours within `delta` and the taper `kind` are found per chunk on the
        device (cocons_krige_taper_apply_delta).  `last_pattern_nnz` then holds the entries the call's pattern had."""
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        m = Xp.shape[0]
        st, qf = np.empty(m), np.empty(m)
        nnz = ctypes.c_longlong(0)
        _lib.check(self._L.cocons_krige_taper_apply_delta(self._h, m, _p(lp), _p(Xp), float(delta), _taper_kind(kind),
                                                          _p(st), _p(qf), ctypes.byref(nnz)),
                   "cocons_krige_taper_apply_delta")
        self.last_pattern_nnz = int(nnz.value)
        return st, qf

    def krige_taper_release(self):
        _lib.check(self._L.cocons_krige_taper_release(self._h), "cocons_krige_taper_release")

    def krige_taper_held(self, theta_list, z_col=0, max_rows=0):
        """`with fit.krige_taper_held(theta_list):` -- krige_taper_prepare on the way in, krige_taper_release on the way out"""
        return _held(self.krige_taper_prepare, self.krige_taper_release, theta_list, z_col, max_rows)

    def krige_taper_info(self):
        """{prepared, bytes, rows, n, W, nt}: whether a state is held, its device bytes, rows per chunk, observations,
        slots of the ring (tile columns of the band), tile columns of the factor."""
        out = (ctypes.c_longlong * 6)()
        _lib.check(self._L.cocons_krige_taper_info(self._h, out), "cocons_krige_taper_info")
        return {"prepared": bool(out[0]), "bytes": int(out[1]), "rows": int(out[2]), "n": int(out[3]), "W": int(out[4]),
                "nt": int(out[5])}

    def krige_taper_joint_core(self, locs_pred, x_covariates_pred, pred_taper, uu_taper, locs_unobs=None, iiderrors=None,
                               cov=True):
        """(stochastic, cov | None, sims | None) at the new locations against the prepared band factor
        (cocons_krige_taper_joint): cov = S_uu - C S^-1 C' (m x m, symmetric to the bit), S_uu = uu_taper o cov_rns_taper at
        locs_unobs (default locs_pred); sims = chol(cov) iiderrors + (X_pred mean + stochastic) for iiderrors m x nsim.
        pred_taper as krige_taper_core takes it; uu_taper = (colindices, rowpointers, entries) of the m x m taper between the
        new locations (1-based CSR, every row with its diagonal; the entries with column <= row are read).  A predictive
        covariance that is not positive definite in floating point (draws only) raises KrigeJointNotPositiveDefinite."""
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        m = Xp.shape[0]
        ci, rp, te = _csr(pred_taper)
        cu, ru, tu = _csr(uu_taper)
        lu = None if locs_unobs is None else _f(np.asarray(locs_unobs, dtype=np.float64)[:, :2])
        E = None if iiderrors is None else _f(np.asarray(iiderrors, dtype=np.float64).reshape(m, -1))
        nsim = 0 if E is None else E.shape[1]
        st = np.empty(m)
        C = np.empty((m, m), order="F") if cov else None
        Y = np.empty((m, nsim), order="F") if nsim > 0 else None
        rc = self._L.cocons_krige_taper_joint(self._h, m, _p(lp), _p(Xp), int(ci.size), _ip(ci), _ip(rp), _p(te),
                                              None if lu is None else _p(lu), int(cu.size), _ip(cu), _ip(ru), _p(tu), _p(st),
                                              None if C is None else _p(C), nsim, None if nsim == 0 else _p(E),
                                              None if Y is None else _p(Y))
        _check_joint(rc, "cocons_krige_taper_joint")
        return st, C, Y

    def krige_taper_joint_bytes(self, m, nsim=0):
        """Device bytes krige_taper_joint_core allocates for m new locations and nsim draws on this handle, the CSR staging
        apart (cocons_krige_taper_joint_bytes): what a caller sizes m by."""
        out = ctypes.c_longlong(0)
        _lib.check(self._L.cocons_krige_taper_joint_bytes(self._h, int(m), int(nsim), ctypes.byref(out)),
                   "cocons_krige_taper_joint_bytes")
        return int(out.value)

    def sim_core(self, theta_list, iiderrors, pivot=None):
        """Fields of the sparse branch of cocoSim (R/sim.R:177-217), n x nsim: (L_P E)[k] + (X mean) scattered to rows
        pivot[k] - 1, L_P L_P' = S[pivot, pivot].  pivot = None: the handle's own order (same distribution, another field
        for the same draws); spam's ordering(chol(ref_taper)): the reference's fields to rounding."""
        E = _f(np.asarray(iiderrors, dtype=np.float64).reshape(self.n, -1))
        T, mean = _table_mean(theta_list)
        piv = None
        if pivot is not None:
            piv = np.ascontiguousarray(np.asarray(pivot).ravel(), dtype=np.int32)
            if piv.size != self.n:
                raise ValueError("pivot must have length n")
        out = np.empty(E.shape, order="F")
        _lib.check(self._L.cocons_sim_taper(self._h, _p(T), _p(mean), E.shape[1], _p(E), None if piv is None else _ip(piv),
                                            _p(out)), "cocons_sim_taper")
        return out

    def order(self):
        """The handle's own order of the observations: 1-based caller indices by position (reverse Cuthill-McKee)."""
        piv = np.empty(self.n, dtype=np.int32)
        _lib.check(self._L.cocons_fit_taper_order(self._h, _ip(piv)), "cocons_fit_taper_order")
        return piv


def cocoSim_sparse(theta_list, locs, X_std, smooth_limits, z, ref_taper, iiderrors, pivot=None, fit=None):
    """Sparse branch of cocoSim, R/sim.R:177-217, from the point where the scaled design matrix, the theta list and
    ref_taper ((colindices, rowpointers, entries)) exist.  `iiderrors` is the n x nsim matrix of N(0,1) draws; with
    pivot = spam::ordering(spam::chol(ref_taper)) the fields equal the reference's to rounding.  The sparse branch has
    no fixed-smoothness override (:141-145 belong to the dense branch).  Returns n x nsim."""
    E = np.asarray(iiderrors, dtype=np.float64)
    n = np.asarray(X_std).shape[0]
    with _tapered(fit, locs, X_std, z, smooth_limits, ref_taper) as f, _chol_error():
        return f.sim_core(theta_list, E.reshape(n, -1), pivot=pivot)


def cocoPredict_sparse(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, ref_taper, pred_taper,
                       type="pred", fit=None):
    """Sparse branch of cocoPredict, R/predict.R:190-283, from the point where the scaled design matrices, the
    adjusted theta list and the two taper matrices (taper_two = ref_taper, pred_taper; (colindices, rowpointers,
    entries) each) exist."""
    with _tapered(fit, locs, X_std, z, smooth_limits, ref_taper) as f:
        st, qf = f.predict_core(theta_list, newlocs, X_pred_std, pred_taper)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def _abs_root(unc):
    """sqrt of the predictive variances under the reference's abs rule below 1e-10 (R/predict.R:175-177, :269-271); `unc`
    is overwritten"""
    neg = unc < 1e-10
    unc[neg] = np.abs(unc[neg])
    return np.sqrt(unc)


def _predict_outputs(theta_list, X_pred_std, st, qf, type):
    """cocoPredict's host lines after the kriging core (R/predict.R:165-183, the same at :247-277 in the sparse branch)."""
    Xp = np.asarray(X_pred_std, dtype=np.float64)
    systematic = Xp @ np.asarray(theta_list["mean"], dtype=np.float64)
    if type == "mean":
        return {"systematic": systematic, "stochastic": st}
    with np.errstate(invalid="ignore"):
        unc = 1 / np.exp(-(Xp @ theta_list["std.dev"])) + np.exp(Xp @ theta_list["nugget"])   # :170-171
    unc = unc - qf                                                                         # :173
    return {"systematic": systematic, "stochastic": st, "sd.pred": _abs_root(unc)}


# The sparse branch's tail had this name of its own.  tests/test_gpu_taper_envelopes.py and tests/test_gpu_taper_sizes.py import
# it in 53 cases (test_prediction, test_held_factor_kriging), and those tests as they stood before the tails became one must
# keep passing against this module: the name goes when a change may rewrite that many cases.
_sparse_predict_tail = _predict_outputs


def _joint_outputs(theta_list, X_pred_std, st, cov):
    """The same for the joint forms: sd.pred from the diagonal of the predictive covariance, which is returned too."""
    out = _predict_outputs(theta_list, X_pred_std, st, None, "mean")
    out.update({"sd.pred": _abs_root(np.diag(cov).copy()), "cov.pred": cov})
    return out


def cocoPredict_sparse_chunked(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, ref_taper, pred_taper,
                               type="pred", fit=None, max_rows=0):
    """cocoPredict_sparse from one held band factor: S(theta) is factored once (krige_taper_prepare) and the new
    locations are predicted in chunks of max_rows rows (0: the library's default) through a ring of the band's tile
    columns -- device memory does not grow with the number of new locations.  Returns what cocoPredict_sparse returns."""
    with _tapered(fit, locs, X_std, z, smooth_limits, ref_taper) as f:
        with f.krige_taper_held(theta_list, max_rows=max_rows):
            st, qf = f.krige_taper_core(newlocs, X_pred_std, pred_taper)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def cocoPredict_sparse_delta(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, ref_taper, delta, kind="wend1",
                             type="pred", fit=None, max_rows=0):
    """cocoPredict_sparse_chunked without pred_taper: the library finds the neighbours of the new locations within `delta`
    and evaluates the taper `kind` itself."""
    with _tapered(fit, locs, X_std, z, smooth_limits, ref_taper) as f:
        with f.krige_taper_held(theta_list, max_rows=max_rows):
            st, qf = f.krige_taper_core_delta(newlocs, X_pred_std, delta, kind)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def cocoPredict_sparse_joint(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, ref_taper, pred_taper, uu_taper,
                             fit=None):
    """cocoPredict_sparse with the predictive covariance BETWEEN the new locations: {"systematic", "stochastic", "sd.pred",
    "cov.pred"}, cov.pred = S_uu - C S^-1 C' (m x m) from one held band factor (krige_taper_prepare,
    krige_taper_joint_core, release), S_uu = uu_taper o cov_rns_taper at the new locations, and sd.pred the root of its
    diagonal with the reference's abs rule below 1e-10 (R/predict.R:269-271).  uu_taper = (colindices, rowpointers,
    entries) of spam::nearest.dist(newlocs, delta, upper = NULL) with the taper applied."""
    with _tapered(fit, locs, X_std, z, smooth_limits, ref_taper) as f:
        with f.krige_taper_held(theta_list):
            st, cov, _ = f.krige_taper_joint_core(newlocs, X_pred_std, pred_taper, uu_taper)
    return _joint_outputs(theta_list, X_pred_std, st, cov)


def cocoSim_cond_sparse_held(theta_list, locs, newlocs, newdataset, X_std, X_pred_std, smooth_limits, z, ref_taper,
                             pred_taper, uu_taper, iiderrors, fit=None):
    """Conditional simulation (sim.type = "cond") of a tapered model, which the reference's cocoSim does not offer for
    sparse objects (R/sim.R:177-217): cocoSim_cond_dense_held's draws from a held band factor -- prepare, one joint call
    (krige_taper_joint_core: only the m x m Cholesky of the predictive covariance is taken), release.  `newdataset`
    supplies the coordinates of S_uu (its first two columns), uu_taper its pattern and taper values.  Returns m x nsim."""
    with _tapered(fit, locs, X_std, z, smooth_limits, ref_taper) as f, \
            _chol_error(KrigeJointNotPositiveDefinite), f.krige_taper_held(theta_list):
        return f.krige_taper_joint_core(newlocs, X_pred_std, pred_taper, uu_taper, np.asarray(newdataset, dtype=np.float64),
                                        iiderrors, cov=False)[2]


def _cv_result(f, z, resid, var):
    z = np.asarray(z, dtype=np.float64).reshape(f.n, -1)
    return {"mean.pred": z - resid, "sd.pred": np.sqrt(var), "resid": resid}


def cocoCV_dense(theta_list, locs, X_std, smooth_limits, z, fold=None, fit=None):
    """Cross-validated predictions of the dense model at `theta_list` from ONE factorisation (cocons_cv_dense) instead of
    one fit per fold.  `fold`: one label of any kind per observation (None: leave-one-out).  Returns `mean.pred` (n x r:
    every observation predicted from the observations outside its fold), `sd.pred` (n, nugget included) and
    `resid` = z - mean.pred -- what getLogScore / getCRPS take.  A failing Cholesky raises CholeskyError."""
    lab = None if fold is None else np.unique(np.asarray(fold).ravel(), return_inverse=True)[1]
    with _dense(fit, locs, X_std, z, smooth_limits) as f:
        return _cv_result(f, z, *f.cv_core(theta_list, lab))


def cocoCV_sparse(theta_list, locs, X_std, smooth_limits, z, ref_taper, fit=None, fold=None):
    """Cross-validated predictions of the tapered model; `ref_taper` = (colindices, rowpointers, entries).  `fold`: one label
    of any kind per observation, every fold from the one held band factor (cocons_cv_taper_folds); None: leave-one-out
    (cocons_cv_taper).  Returns what `cocoCV_dense` returns."""
    lab = None if fold is None else np.unique(np.asarray(fold).ravel(), return_inverse=True)[1]
    with _tapered(fit, locs, X_std, z, smooth_limits, ref_taper) as f:
        return _cv_result(f, z, *f.cv_core(theta_list, lab))


def _pnorm(x):
    from math import erf
    return 0.5 * (1.0 + np.vectorize(erf)(np.asarray(x, dtype=np.float64) / np.sqrt(2.0)))


def getLogScore(z_pred, mean_pred, sd_pred):
    """R/getFunctions.R:100-104: the logarithmic score of Gaussian predictions, elementwise."""
    z, m, s = (np.asarray(a, dtype=np.float64) for a in (z_pred, mean_pred, sd_pred))
    return (np.log(2 * np.pi) + ((z - m) / s) ** 2) / 2 + np.log(s)


def getCRPS(z_pred, mean_pred, sd_pred):
    """R/getFunctions.R:117-124: the continuous ranked probability score of Gaussian predictions, elementwise."""
    z, m, s = (np.asarray(a, dtype=np.float64) for a in (z_pred, mean_pred, sd_pred))
    t = (m - z) / s
    return s * (t * (2 * _pnorm(t) - 1) + 2 * np.exp(-0.5 * t * t) / np.sqrt(2 * np.pi) - 1 / np.sqrt(np.pi))


def _objective(theta, par_pos, lam, smooth_limits, safe, handle, core, dof, grad=False, sd0_profiled=False):
    """The frame of every GetNeg2loglikelihood* wrapper (R/neg2loglikelihood.R:183-222 and its siblings): theta through
    getModelLists(type="diff"), `core(f, tl)` on the handle that `handle` (a `_borrowed`) yields, the penalty of
    N = dof * r observations added.  A failing Cholesky inside `core` gives 1e6 under `safe` (:202-206) and
    RuntimeError("Cholesky error") otherwise.

    grad = False: `core` returns the value without the penalty.  grad = True: it returns (value, tables, grad_mean) --
    6 x p tables in the order of COV_ASPECTS, added to the penalty's gradient one after the other, and the mean's gradient
    (None where the mean is profiled out) -- and the frame returns (value, the gradient over the optimiser's vector through
    getModelLists_grad); after a failing Cholesky (1e6, zeros) under `safe`.

    sd0_profiled: std.dev[0] = 0 after getModelLists, the marginal variance profiled out (:80); its gradient entry is 0."""
    tl = getModelLists(theta, par_pos, "diff")
    if sd0_profiled:
        sd = np.array(tl["std.dev"], dtype=np.float64, copy=True)
        sd[0] = 0.0
        tl["std.dev"] = sd
    with handle as f:
        try:
            out = core(f, tl)
        except CholeskyError:
            if safe:
                return (1e6, np.zeros(np.asarray(theta).size)) if grad else 1e6
            raise RuntimeError("Cholesky error")
        N = dof * f.r
        if not grad:
            return out + getPen(N, lam, tl, smooth_limits)
        val, tables, gm = out
        g = getPen_grad(N, lam, tl, smooth_limits)
        if gm is not None:
            g["mean"] = g["mean"] + gm
        for table in tables:
            for t, k in enumerate(COV_ASPECTS):
                g[k] = g[k] + table[t]
        if sd0_profiled:
            g["std.dev"][0] = 0.0
        return val + getPen(N, lam, tl, smooth_limits), getModelLists_grad(g, par_pos)


def _profile_value(parts, r, n):
    """R/neg2loglikelihood.R:102-106 without the penalty, from parts = (logdet, the r quadratic forms): (value, their sum Q)"""
    logdet, sum_in = parts[0], float(np.sum(parts[1:]))
    return r * n * np.log(2 * np.pi) + r * n + r * 2 * logdet + r * n * np.log(sum_in / (r * n)), sum_in


def GetNeg2loglikelihoodTaper(theta, par_pos, ref_taper, locs, x_covariates, smooth_limits, z, n, lam, safe=True,
                              fit=None):
    """R/neg2loglikelihood.R:20-53.  `ref_taper` = (colindices, rowpointers, entries) of the spam taper matrix;
    `fit` (optional) a CoconsTaperFit built once from the same data.  cholS has no counterpart: the factorisation
    is dense."""
    return _objective(theta, par_pos, lam, smooth_limits, safe, _tapered(fit, locs, x_covariates, z, smooth_limits, ref_taper),
                      lambda f, tl: f.neg2loglik_core(tl)[0], n)


def GetNeg2loglikelihoodTaperProfile(theta, par_pos, ref_taper, locs, x_covariates, smooth_limits, z, n, lam,
                                     safe=True, fit=None):
    """R/neg2loglikelihood.R:73-108: std.dev[1] = 0, the marginal variance profiled out."""
    return _objective(theta, par_pos, lam, smooth_limits, safe, _tapered(fit, locs, x_covariates, z, smooth_limits, ref_taper),
                      lambda f, tl: _profile_value(f.neg2loglik_core(tl)[1], f.r, n)[0], n, sd0_profiled=True)


def GetNeg2loglikelihoodTaper_grad(theta, par_pos, ref_taper, locs, x_covariates, smooth_limits, z, n, lam, safe=True,
                                   fit=None):
    """`GetNeg2loglikelihoodTaper` and its gradient over the optimiser's vector `theta` in one call: (value, gradient).
    The gradient is that of the tapered -2 log-likelihood (cocons_neg2loglik_grad_taper) plus the penalty's, carried
    through getModelLists(type="diff").  A failing Cholesky gives (1e6, zeros) under `safe`, RuntimeError otherwise."""
    def core(f, tl):
        val, _, gt, _, gm = f.neg2loglik_grad_core(tl)
        return val, (gt,), gm

    return _objective(theta, par_pos, lam, smooth_limits, safe, _tapered(fit, locs, x_covariates, z, smooth_limits, ref_taper),
                      core, n, grad=True)


def GetNeg2loglikelihoodTaperProfile_grad(theta, par_pos, ref_taper, locs, x_covariates, smooth_limits, z, n, lam,
                                          safe=True, fit=None):
    """`GetNeg2loglikelihoodTaperProfile` and its gradient over `theta`: (value, gradient).  With Q the sum of the quadratic
    forms the value is r 2 logdet + r n log(Q / (r n)) + constants, so its gradient is the log-determinant's part of the
    core's plus r n / Q times the quadratic forms' part (the mean gradient scaled likewise).  std.dev[0] is overwritten
    with 0 after getModelLists: its table gradient is zero (where std.dev and scale are both free the raw pair still
    moves scale[0])."""
    def core(f, tl):
        _, parts, gt, gq, gm = f.neg2loglik_grad_core(tl)
        val, sum_in = _profile_value(parts, f.r, n)
        w = f.r * n / sum_in
        return val, (gt - gq, w * gq), w * gm

    return _objective(theta, par_pos, lam, smooth_limits, safe, _tapered(fit, locs, x_covariates, z, smooth_limits, ref_taper),
                      core, n, grad=True, sd0_profiled=True)


def GetNeg2loglikelihood(theta, par_pos, locs, x_covariates, smooth_limits, z, n, lam, safe=True, fit=None):
    """R/neg2loglikelihood.R:183-222.  `fit` (optional) is a CoconsFit built once from the
    same (locs, x_covariates, z, smooth_limits); without it the data are uploaded per call."""
    return _objective(theta, par_pos, lam, smooth_limits, safe, _dense(fit, locs, x_covariates, z, smooth_limits),
                      lambda f, tl: f.neg2loglik_core(tl)[0], n)


def GetNeg2loglikelihood_grad(theta, par_pos, locs, x_covariates, smooth_limits, z, n, lam, safe=True, fit=None):
    """`GetNeg2loglikelihood` and its gradient over the optimiser's vector `theta` in one call: (value, gradient).  The
    value agrees with GetNeg2loglikelihood's to about 1e-12 relative (the same objective, factored on the plain schedule
    rather than the dependency-driven one: another summation order); the gradient is that of the -2 log-likelihood
    (cocons_neg2loglik_grad_dense) plus the penalty's, carried through getModelLists(type="diff").  A failing Cholesky
    gives (1e6, zeros) under `safe`, RuntimeError("Cholesky error") otherwise."""
    def core(f, tl):
        val, _, gt, gm = f.neg2loglik_grad_core(tl)
        return val, (gt,), gm

    return _objective(theta, par_pos, lam, smooth_limits, safe, _dense(fit, locs, x_covariates, z, smooth_limits), core, n,
                      grad=True)


def GetNeg2loglikelihood_batch(thetas, par_pos, locs, x_covariates, smooth_limits, z, n, lam, safe=True, fit=None):
    """`GetNeg2loglikelihood` at several theta vectors at once -- what optimParallel's workers
    compute in parallel for one gradient (R/optim.R:237-259).  Same values, same `safe` rule."""
    tls = [getModelLists(t, par_pos, "diff") for t in thetas]
    with _dense(fit, locs, x_covariates, z, smooth_limits) as f:
        vals, st = f.neg2loglik_batch_core(tls)
        out = np.empty(len(tls))
        for i, tl in enumerate(tls):
            if st[i] > 0:
                if not safe:
                    raise RuntimeError("Cholesky error")
                out[i] = 1e6
            else:
                out[i] = vals[i] + getPen(n * f.r, lam, tl, smooth_limits)
        return out


def getHessian_dense(par, par_pos, locs, x_covariates, smooth_limits, z, n, lam, f00=None,
                      eps=np.finfo(float).eps ** 0.25, fit=None):
    """Dense branch of getHessian, R/getFunctions.R:925-1034, from the point where the scaled
    design matrix exists: for every index pair (jj <= ii) three objective values at par shifted by
    eps, H[jj,ii] = 0.5 (f11 - f01 - f10 + f00) / eps^2, then H + t(H) with the diagonal halved.
    The reference farms the 3 P (P+1)/2 evaluations out with parApply (:979); here they form one
    pipelined batch on the GPU."""
    par = np.asarray(par, dtype=np.float64).ravel()
    P = par.size
    with _dense(fit, locs, x_covariates, z, smooth_limits) as f:
        if f00 is None:
            f00 = GetNeg2loglikelihood(par, par_pos, locs, x_covariates, smooth_limits, z, n, lam, fit=f)
        pts, idx = [], []
        for jj in range(P):
            for ii in range(jj, P):
                t01, t10, t11 = par.copy(), par.copy(), par.copy()
                t01[jj] += eps
                t10[ii] += eps
                t11[jj] += eps
                t11[ii] += eps
                pts += [t01, t10, t11]
                idx.append((jj, ii))
        vals = GetNeg2loglikelihood_batch(pts, par_pos, locs, x_covariates, smooth_limits, z, n, lam, fit=f)
        H = np.zeros((P, P))
        for k, (jj, ii) in enumerate(idx):
            f01, f10, f11 = vals[3 * k], vals[3 * k + 1], vals[3 * k + 2]
            H[jj, ii] = 0.5 * ((f11 - f01 - f10 + f00) / (eps * eps))
        H = H + H.T
        H[np.diag_indices(P)] /= 2
        return H


def fisher_jacobian(par, par_pos):
    """The optimiser's vector maps affinely onto the mean and the 6 x p table (getModelLists(type="diff")), so row a of the
    Jacobian is getModelLists(par + e_a) - getModelLists(par), exactly.  Returns (J_table P x 6p, J_mean P x p)."""
    par = np.asarray(par, dtype=np.float64).ravel()
    base = getModelLists(par, par_pos, "diff")
    T0, m0 = theta_table(base), np.asarray(base["mean"], dtype=np.float64)
    Jt, Jm = np.zeros((par.size, T0.size)), np.zeros((par.size, m0.size))
    for a in range(par.size):
        e = par.copy()
        e[a] += 1.0
        tl = getModelLists(e, par_pos, "diff")
        Jt[a] = (theta_table(tl) - T0).ravel()
        Jm[a] = np.asarray(tl["mean"], dtype=np.float64) - m0
    return Jt, Jm


def fisher_to_par(info_table, info_mean, par, par_pos):
    """An information matrix over the table's 6p entries (and the p x p mean block; the block between them is 0) in the
    optimiser's coordinates: J_t I_table J_t' + J_m I_mean J_m', rows and columns in `par`'s order."""
    Jt, Jm = fisher_jacobian(par, par_pos)
    return Jt @ np.asarray(info_table, dtype=np.float64) @ Jt.T + Jm @ np.asarray(info_mean, dtype=np.float64) @ Jm.T


def _fisher_in_par(par, par_pos, handle, probes=None, grouped=False):
    """A handle's `fisher_core` in the optimiser's coordinates: the rows of `fisher_jacobian` that move the table go to the
    device as directions (a pure mean parameter costs nothing there), J_m info_mean J_m' is added for the mean; the block
    between them is 0.  `handle`: a `_borrowed`; `probes(f)`: the probes a tapered handle's core takes; `grouped`: a Vecchia
    handle's core on the grouped schedule."""
    par = np.asarray(par, dtype=np.float64).ravel()
    tl = getModelLists(par, par_pos, "diff")
    Jt, Jm = fisher_jacobian(par, par_pos)
    with handle as f:
        more = {} if probes is None else {"probes": probes(f)}
        if grouped:
            more["grouped"] = True
        cov = np.flatnonzero(np.any(Jt != 0, axis=1))
        sub, info_mean = f.fisher_core(tl, Jt[cov] if cov.size else Jt[:1], **more)
        info = Jm @ info_mean @ Jm.T
        if cov.size:
            info[np.ix_(cov, cov)] += sub
        return info


def getFisher_dense(par, par_pos, locs, x_covariates, smooth_limits, z, n, fit=None):
    """The P x P expected (Fisher) information of the dense model in the optimiser's coordinates, rows and columns in
    `par`'s order, from ONE factorisation (cocons_fisher_dense) instead of getHessian_dense's 3 P (P + 1) / 2 evaluations.

    What it is: the expected Hessian of the negative log-likelihood -l at the model, i.e. E[getHessian] in the reference's
    own convention (0.5 (f11 - f01 - f10 + f00) / eps^2 is the Hessian of -l), positive semi-definite by construction, so
    solve() of it gives non-negative variances.  What it is not: it contains no penalty (lambda plays no part), and it is
    not the observed Hessian -- at the data actually drawn the two differ by a term of zero mean.

    The Jacobian rows of `fisher_jacobian` go to the device as directions; the mean part is J_m (r X' Sigma^-1 X) J_m';
    the block between mean and covariance parameters is 0.  A failing Cholesky raises CholeskyError."""
    return _fisher_in_par(par, par_pos, _dense(fit, locs, x_covariates, z, smooth_limits))


def getFisher_reml(par, par_pos, locs, x_covariates, x_betas, smooth_limits, z, n, fit=None):
    """The P x P expected information of the REML fit in the optimiser's coordinates, rows and columns in `par`'s order,
    from ONE factorisation (cocons_fisher_reml): (r / 2) tr(P Sigma_a P Sigma_b) with the REML projector P, the expected
    Hessian of half of what `GetNeg2loglikelihoodREML` returns, without the penalty.  The reference has no counterpart
    (getHessian stops for reml objects); solve() of the result is the inv.hess of getCIs / getModHess.

    `x_betas` is accepted and unused, as in `GetNeg2loglikelihoodREML`.  REML has no mean parameters: a free entry of
    `par_pos["mean"]` raises ValueError.  A failing Cholesky raises CholeskyError."""
    par = np.asarray(par, dtype=np.float64).ravel()
    tl = getModelLists(par, par_pos, "diff")
    Jt, Jm = fisher_jacobian(par, par_pos)
    if np.any(Jm != 0):
        raise ValueError("getFisher_reml: par_pos has a free mean entry; the REML objective has no mean parameters")
    with _dense(fit, locs, x_covariates, z, smooth_limits) as f:
        return f.fisher_reml_core(tl, Jt)


def getFisher_sparse(par, par_pos, locs, x_covariates, smooth_limits, z, n, ref_taper, nprobe=0, seed=0, fit=None):
    """The P x P expected (Fisher) information of the tapered model (type = "sparse") in the optimiser's coordinates, rows
    and columns in `par`'s order, on the band factor of one factorisation (cocons_fisher_taper): (r / 2) tr(S^-1 S_a S^-1 S_b)
    with S = T o C(theta), plus J_m (r X' S^-1 X) J_m' for the mean.  It is to `GetNeg2loglikelihoodTaper` what
    `getFisher_dense` is to the dense objective -- the expectation of what the sparse branch of getHessian estimates from
    3 P (P + 1) / 2 + 1 objective values -- a Gram matrix, hence symmetric and positive semi-definite; no penalty, not the
    observed Hessian.  `ref_taper` = (colindices, rowpointers, entries).

    nprobe = 0 is exact: the n unit vectors are run through the band factor, which costs O(ndir n^2 bandwidth) -- 0.2 s
    at n = 10^4, a minute and a half at n = 10^5.  nprobe > 0 draws that many Rademacher probes from
    numpy.random.default_rng(seed) and returns Hutchinson's estimate (the trace self-averages over the sites: 64 probes
    came within 1 - 2 % of sqrt(I_aa I_bb) at n ~ 10^3, 0.5 % at 10^4, 0.2 % at 10^5); the mean block is exact either way.
    The Profile form (`GetNeg2loglikelihoodTaperProfile`) has no counterpart here.  A failing Cholesky raises
    CholeskyError."""
    def probes(f):
        if nprobe > 0:
            return np.random.default_rng(seed).integers(0, 2, size=(f.n, int(nprobe))) * 2.0 - 1.0

    return _fisher_in_par(par, par_pos, _tapered(fit, locs, x_covariates, z, smooth_limits, ref_taper), probes)


def GetNeg2loglikelihoodProfile(theta, par_pos, locs, x_covariates, smooth_limits, z, n, x_betas, lam,
                                safe=True, fit=None):
    """R/neg2loglikelihood.R:127-165."""
    return _objective(theta, par_pos, lam, smooth_limits, safe, _dense(fit, locs, x_covariates, z, smooth_limits, x_betas),
                      lambda f, tl: f.neg2loglik_profile_core(tl)[0], n)


def GetNeg2loglikelihoodREML(theta, par_pos, locs, x_covariates, x_betas, smooth_limits, z, n, lam,
                             safe=True, fit=None):
    """R/neg2loglikelihood.R:241-291 (x_betas is accepted and, as in the reference, unused)."""
    rank = int(np.linalg.matrix_rank(np.asarray(x_covariates, dtype=np.float64)))   # qr(x)$rank, :270
    return _objective(theta, par_pos, lam, smooth_limits, safe, _dense(fit, locs, x_covariates, z, smooth_limits),
                      lambda f, tl: f.neg2loglik_reml_core(tl, rank)[0], n - rank)


def GetNeg2loglikelihoodProfile_grad(theta, par_pos, locs, x_covariates, smooth_limits, z, n, x_betas, lam,
                                     safe=True, fit=None):
    """`GetNeg2loglikelihoodProfile` and its gradient over the optimiser's vector in one call: (value, gradient)
    (cocons_neg2loglik_profile_grad; the mean is profiled out, so `par_pos["mean"]` holds no free entry)."""
    def core(f, tl):
        val, _, gt = f.neg2loglik_profile_grad_core(tl)
        return val, (gt,), None

    return _objective(theta, par_pos, lam, smooth_limits, safe, _dense(fit, locs, x_covariates, z, smooth_limits, x_betas),
                      core, n, grad=True)


def GetNeg2loglikelihoodREML_grad(theta, par_pos, locs, x_covariates, x_betas, smooth_limits, z, n, lam,
                                  safe=True, fit=None):
    """`GetNeg2loglikelihoodREML` and its gradient over the optimiser's vector in one call: (value, gradient)
    (cocons_neg2loglik_reml_grad; x_betas is accepted and unused, as there)."""
    rank = int(np.linalg.matrix_rank(np.asarray(x_covariates, dtype=np.float64)))

    def core(f, tl):
        val, _, gt = f.neg2loglik_reml_grad_core(tl, rank)
        return val, (gt,), None

    return _objective(theta, par_pos, lam, smooth_limits, safe, _dense(fit, locs, x_covariates, z, smooth_limits), core,
                      n - rank, grad=True)


def getBetas_profile(theta_list, locs, x_covariates, smooth_limits, z, x_betas, fit=None):
    """The "Compute Betas" block of cocoOptim's pml/reml branch, R/optim.R:329-341:
    solve(W, t(V)) %*% rowSums(z) / ncol(z) with V = Sigma^-1 x_betas, W = x_betas' V -- here read
    off the Gram matrix of the bordered factorisation (no second Cholesky, no V)."""
    with _dense(fit, locs, x_covariates, z, smooth_limits, x_betas) as f, _chol_error():
        _, parts = f.neg2loglik_profile_core(theta_list)
        return parts[2 + f.r: 2 + f.r + f.q].copy()


def cocoSim_dense(theta_list, locs, X_std, smooth_limits, iiderrors, type="classic", fit=None):
    """Marginal branch of cocoSim for a dense object, R/sim.R:147-172, from the point where the
    scaled design matrix and the theta list exist.  `iiderrors` is the n x nsim matrix of N(0,1)
    draws (the reference draws it with rnorm after set.seed; pass the same numbers for identical
    output).  type = "classic" -> cov_rns_classic, "diff" -> cov_rns.  Returns n x nsim."""
    if type not in ("classic", "diff"):
        raise ValueError("type must be 'classic' or 'diff'")
    E = np.asarray(iiderrors, dtype=np.float64)
    n = np.asarray(X_std).shape[0]
    with _dense(fit, locs, X_std, np.zeros(n), smooth_limits) as f, _chol_error():
        return f.sim_core(theta_list, E.reshape(n, -1), classic=(type == "classic"))


def cocoSim_cond_dense(theta_list, locs, newlocs, newdataset, X_std, X_pred_std, smooth_limits, z, iiderrors,
                       fit=None):
    """Conditional branch of cocoSim (sim.type = "cond") for a dense object, R/sim.R:69-127, from the
    point where the scaled design matrices and the theta list exist.  `newdataset` supplies the
    coordinates of covmat_unobs exactly as the reference passes it (`locs = as.matrix(newdataset)`,
    i.e. its first two columns, :96-99).  Returns m x nsim."""
    with _dense(fit, locs, X_std, z, smooth_limits) as f, _chol_error():
        return f.sim_cond_core(theta_list, newlocs, X_pred_std, np.asarray(newdataset, dtype=np.float64), iiderrors)


def cocoSim_cond_dense_held(theta_list, locs, newlocs, newdataset, X_std, X_pred_std, smooth_limits, z, iiderrors,
                            fit=None):
    """cocoSim_cond_dense from a held factor of Sigma(theta): prepare, one joint call (krige_joint_core: the predictive
    covariance is formed from the factor, and only its own m x m Cholesky is taken), release.  Same arguments and output
    as cocoSim_cond_dense; the handle's kriging state is released on return."""
    with _dense(fit, locs, X_std, z, smooth_limits) as f, _chol_error(KrigeJointNotPositiveDefinite), \
            f.krige_held(theta_list):
        return f.krige_joint_core(newlocs, X_pred_std, np.asarray(newdataset, dtype=np.float64), iiderrors, cov=False)[2]


def cocoPredict_dense(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, type="pred", fit=None):
    """Dense branch of cocoPredict, R/predict.R:136-187, from the point where the scaled
    design matrices and the adjusted theta list exist."""
    with _dense(fit, locs, X_std, z, smooth_limits) as f:
        st, qf = f.predict_core(theta_list, newlocs, X_pred_std)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def cocoPredict_dense_chunked(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, type="pred", fit=None,
                              max_rows=0):
    """cocoPredict_dense from one held factor: Sigma(theta) is factored once (krige_prepare) and the new locations are
    predicted in chunks of at most max_rows rows (0: the library's default), so that device memory does not grow with
    their number.  Same arguments and outputs as cocoPredict_dense; the handle's kriging state is released on return."""
    with _dense(fit, locs, X_std, z, smooth_limits) as f:
        with f.krige_held(theta_list, max_rows=max_rows):
            st, qf = f.krige_core(newlocs, X_pred_std)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def cocoPredict_dense_joint(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, fit=None):
    """cocoPredict_dense with the predictive covariance BETWEEN the new locations: {"systematic", "stochastic", "sd.pred",
    "cov.pred"}, cov.pred = Sigma_uu - C Sigma^-1 C' (m x m) from one held factor (krige_prepare, krige_joint_core,
    release) and sd.pred the root of its diagonal with the reference's abs rule below 1e-10 (R/predict.R:175-177)."""
    with _dense(fit, locs, X_std, z, smooth_limits) as f:
        with f.krige_held(theta_list):
            st, cov, _ = f.krige_joint_core(newlocs, X_pred_std)
    return _joint_outputs(theta_list, X_pred_std, st, cov)


# --------------------------------------------------------------------------- #
# Vecchia approximation: the model's own likelihood from n small blocks, O(n m) memory
# --------------------------------------------------------------------------- #
def _nn_table(nn, rows):
    nn = np.asarray(nn, dtype=np.int32)
    if nn.ndim != 2:
        nn = nn.reshape(rows, -1)
    if nn.shape[0] != rows:
        raise ValueError("the neighbour table must have one row per location")
    return np.asfortranarray(nn), int(nn.shape[1])


def vecchia_neighbours(locs, m) -> np.ndarray:
    """The exact m nearest EARLIER observations of every row of locs (n x 2), in the order the rows come in (the Vecchia
    order: choosing it -- maxmin, random, by coordinate -- stays with the caller): n x m int32 in Fortran order, 1-based,
    nearest first, ties broken by index, zero-padded where a row has fewer than m predecessors.  The first rows by brute
    force; the rows [b / 2, b) of every doubling block from a k-d tree over the first b points, queried with a doubling k
    until m earlier points are found and every point tied with the last of them has been seen."""
    from scipy.spatial import cKDTree
    locs = np.ascontiguousarray(np.asarray(locs, dtype=np.float64))
    n, m = locs.shape[0], int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    nn = np.zeros((n, m), dtype=np.int32, order="F")

    def dist(rows, idx):
        return np.hypot(locs[idx, 0] - locs[rows, 0][:, None], locs[idx, 1] - locs[rows, 1][:, None])

    head = min(n, max(2 * m + 1, 64))
    for i in range(1, head):
        o = np.lexsort((np.arange(i), dist(np.array([i]), np.arange(i)[None, :])[0]))[:m]
        nn[i, :o.size] = o + 1
    lo = head
    while lo < n:
        hi = min(n, 2 * lo)
        tree = cKDTree(locs[:hi])
        for b0 in range(lo, hi, 65536):
            todo = np.arange(b0, min(hi, b0 + 65536))
            k = min(hi, 2 * m + 2)
            while todo.size:
                idx = np.asarray(tree.query(locs[todo], k=k)[1]).reshape(todo.size, -1)
                d = dist(todo, idx)
                earlier = idx < todo[:, None]
                dm = np.where(earlier, d, np.inf)
                order = np.lexsort((idx, dm), axis=1)[:, :m]
                far = np.take_along_axis(dm, order[:, -1:], axis=1)[:, 0]      # the m-th earlier point (inf: fewer than m)
                done = np.isfinite(far) & ((k == hi) | (np.max(d, axis=1) > far))
                nn[todo[done], :] = np.take_along_axis(idx, order, axis=1)[done] + 1
                todo = todo[~done]
                k = min(hi, 2 * k)
        lo = hi
    return nn


def vecchia_neighbours_pred(locs, newlocs, m) -> np.ndarray:
    """The m nearest observations of every new location (plain kNN): mp x m int32 in Fortran order, 1-based, zero-padded
    when there are fewer than m observations."""
    from scipy.spatial import cKDTree
    locs = np.ascontiguousarray(np.asarray(locs, dtype=np.float64))
    new = np.ascontiguousarray(np.asarray(newlocs, dtype=np.float64))
    n, m = locs.shape[0], int(m)
    k = min(n, m)
    _, idx = cKDTree(locs).query(new, k=k)
    nn = np.zeros((new.shape[0], m), dtype=np.int32, order="F")
    nn[:, :k] = np.asarray(idx).reshape(new.shape[0], k) + 1
    return nn


def _neighbours_device(locs, newlocs, m, device):
    L = _lib.load()
    locs = _f(locs)
    n = locs.shape[0]
    q = None if newlocs is None else _f(newlocs)
    rows = n if q is None else q.shape[0]
    nn = np.zeros((rows, int(m)), dtype=np.int32, order="F")
    _lib.check(L.cocons_vecchia_neighbours(n, _p(locs), 0 if q is None else rows, None if q is None else _p(q), int(m),
                                           int(device), _ip(nn)), "cocons_vecchia_neighbours")
    return nn


def vecchia_neighbours_device(locs, m, device=0) -> np.ndarray:
    """`vecchia_neighbours` found on the device (cocons_vecchia_neighbours): n x m int32 in Fortran order,
    1-based, nearest first, zero-padded.  The rule is the key (d2, index) with d2 = dx dx + dy dy in fp64, no square root,
    ties to the lower index; `vecchia_neighbours` ranks by np.hypot, which rounds near-ties differently, so the two tables
    may differ in rows that hold such ties (a regular lattice with an inexact spacing)."""
    return _neighbours_device(locs, None, m, device)


def vecchia_neighbours_pred_device(locs, newlocs, m, device=0) -> np.ndarray:
    """`vecchia_neighbours_pred` found on the device, by the rule of `vecchia_neighbours_device`: mp x m int32 in Fortran
    order, 1-based, nearest first, zero-padded when there are fewer than m observations."""
    return _neighbours_device(locs, newlocs, m, device)


def vecchia_neighbours_corr(S, nn_cand, m, hops=2) -> np.ndarray:
    """The Vecchia neighbours by model correlation (the rule: include/cocons_hip.h), restated on the host:
    S the n x n covariance of the observations at theta in the Vecchia order (`cov_rns`), nn_cand the Euclidean ordered table
    (n x m_cand, 1-based, 0 = none; `vecchia_neighbours_device`).  The candidates of row i are nn_cand's row i and, with
    hops = 2, the rows of its members, each index once; row i lists the m of them with the largest key (rho, then the lower
    index), rho = S[j, i] / sqrt(S[i, i] S[j, j]) with one rounding per operation, compared by the total order of its bit
    patterns (for rho >= 0: by value): n x m int32 in Fortran order, 1-based, largest rho first, zero-padded.  ValueError
    names the first row with a rho that is not finite."""
    S = np.asarray(S, dtype=np.float64)
    n, m, hops = S.shape[0], int(m), int(hops)
    cand = np.asarray(nn_cand, dtype=np.int64).reshape(n, -1)
    if hops not in (1, 2) or m < 1:
        raise ValueError("hops must be 1 or 2 and m at least 1")
    d = np.ascontiguousarray(np.diagonal(S))
    out = np.zeros((n, m), dtype=np.int32, order="F")
    top = np.uint64(1) << np.uint64(63)
    for i in range(n):
        c = cand[i][cand[i] > 0]
        if hops == 2 and c.size:
            c = np.concatenate([c, cand[c - 1].ravel()])
        c = np.unique(c[c > 0]) - 1
        if not c.size:
            continue
        rho = S[c, i] / np.sqrt(d[i] * d[c])
        if not np.all(np.isfinite(rho)):
            raise ValueError("row %d has a candidate whose correlation is not finite" % (i + 1))
        b = rho.view(np.uint64)
        key = ~np.where(b >> np.uint64(63) != 0, ~b, b | top)          # ascends as rho descends
        o = np.lexsort((c, key))[:m]
        out[i, :o.size] = c[o] + 1
    return out


def vecchia_neighbours_corr_pred(Cq, dq, d, nn_pred, nn_all, m, hops=2) -> np.ndarray:
    """The neighbours of NEW locations by model correlation (the rule: include/cocons_hip.h), restated on the
    host: Cq the mp x n cross-covariance of the new locations with the observations at theta (`cov_rns_pred`), dq (mp) and
    d (n) the diagonal values of the prediction branch -- `cov_rns_pred`'s entries for the new locations, and for the
    observations, predicted onto themselves --, nn_pred the plain kNN table of the new locations among all observations
    (mp x m_cand, 1-based, 0 = none; `vecchia_neighbours_pred_device(locs, newlocs, m_cand)`) and nn_all that of the
    observations' own coordinates (n x m_cand; `vecchia_neighbours_pred_device(locs, locs, m_cand)`; read with hops = 2
    only).  The candidates of row q are nn_pred's row q and, with hops = 2, the rows of nn_all that its members name, each
    index once; row q lists the m of them with the largest key (rho, then the lower index), rho = Cq[q, j] / sqrt(dq[q] d[j])
    with one rounding per operation, compared by the total order of its bit patterns: mp x m int32 in Fortran order,
    1-based, largest rho first, zero-padded.  ValueError names the first row with a rho that is not finite."""
    Cq = np.asarray(Cq, dtype=np.float64)
    mp, m, hops = Cq.shape[0], int(m), int(hops)
    dq, d = np.asarray(dq, dtype=np.float64).reshape(mp), np.asarray(d, dtype=np.float64).reshape(Cq.shape[1])
    first = np.asarray(nn_pred, dtype=np.int64).reshape(mp, -1)
    if hops not in (1, 2) or m < 1:
        raise ValueError("hops must be 1 or 2 and m at least 1")
    lists = np.asarray(nn_all, dtype=np.int64).reshape(Cq.shape[1], -1) if hops == 2 else None
    out = np.zeros((mp, m), dtype=np.int32, order="F")
    top = np.uint64(1) << np.uint64(63)
    for q in range(mp):
        c = first[q][first[q] > 0]
        if hops == 2 and c.size:
            c = np.concatenate([c, lists[c - 1].ravel()])
        c = np.unique(c[c > 0]) - 1
        if not c.size:
            continue
        rho = Cq[q, c] / np.sqrt(dq[q] * d[c])
        if not np.all(np.isfinite(rho)):
            raise ValueError("row %d has a candidate whose correlation is not finite" % (q + 1))
        b = rho.view(np.uint64)
        key = ~np.where(b >> np.uint64(63) != 0, ~b, b | top)          # ascends as rho descends
        o = np.lexsort((c, key))[:m]
        out[q, :o.size] = c[o] + 1
    return out


_ORDER_LEVELS = 64
_ORDER_MIX = (0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35)


def _order_labels(n) -> np.ndarray:
    """label(i) for i = 0 .. n - 1 (include/cocons_hip.h, the rule's step 1): three multiply-xorshift rounds on b-bit
    words, walked until the word is below n."""
    b = max(1, int(n - 1).bit_length())
    mask, s = np.uint64((1 << b) - 1), np.uint64((b + 1) // 2)

    def mix(v):
        for c in _ORDER_MIX:
            v = (v * np.uint64(c)) & mask
            v = v ^ (v >> s)
        return v

    v = mix(np.arange(n, dtype=np.uint64))
    while True:
        out = v >= np.uint64(n)
        if not out.any():
            return v.astype(np.int64)
        v[out] = mix(v[out])


def vecchia_order(locs, levels=False):
    """The maxmin ordering by scale-halving nets on the host: the rule of include/cocons_hip.h in numpy, with
    a k-d tree that only proposes candidates -- every decision is the rule's d2 = dx dx + dy dy < e_k.  Returns the order
    (n int32, 1-based: order[t] is the row at position t + 1), with levels=True also the level counts
    [level 0, levels 1 .. K, the rest].  `vecchia_order_device` returns the same bits."""
    from scipy.spatial import cKDTree
    locs = np.ascontiguousarray(np.asarray(locs, dtype=np.float64))
    n = locs.shape[0]
    if n < 1 or locs.shape != (n, 2) or not np.all(np.isfinite(locs)):
        raise ValueError("locs must be n x 2, n >= 1, finite")
    lab = _order_labels(n)
    P = np.empty_like(locs)
    P[lab] = locs                                   # the points in label order: a lower index is a higher priority
    orig = np.empty(n, dtype=np.int64)
    orig[lab] = np.arange(n)
    x0, y0 = locs.min(axis=0)
    x1, y1 = locs.max(axis=0)
    L = max(x1 - x0, y1 - y0)
    c = np.array([x0 + 0.5 * (x1 - x0), y0 + 0.5 * (y1 - y0)])

    def d2(a, b):
        dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
        return dx * dx + dy * dy

    first = int(np.argmin(d2(locs, c)))             # argmin: the first of equal keys, the lower caller's index
    done = [np.array([lab[first]])]
    counts = [1]
    rem = np.delete(np.arange(n), lab[first])
    for k in range(1, _ORDER_LEVELS + 1):
        if rem.size == 0:
            break
        ell = math.ldexp(L, 1 - k)
        e, r = ell * ell, ell * (1.0 + 1e-9)
        taken = []
        if r > 0.0:
            tree = cKDTree(P[rem])
            alive = np.ones(rem.size, dtype=bool)
            S = np.concatenate(done)
            hits = tree.query_ball_point(P[S], r)
            src = np.repeat(np.arange(S.size), [len(h) for h in hits])
            if src.size:
                dst = np.concatenate([np.asarray(h, dtype=np.int64) for h in hits if len(h)])
                alive[dst[d2(P[S[src]], P[rem[dst]]) < e]] = False
            for j in np.flatnonzero(alive):         # ascending label; alive shrinks while the walk goes on
                if not alive[j]:
                    continue
                taken.append(j)
                near = np.asarray(tree.query_ball_point(P[rem[j]], r), dtype=np.int64)
                alive[near[d2(P[rem[near]], P[rem[j]]) < e]] = False
                alive[j] = False
            taken = np.asarray(taken, dtype=np.int64)
        else:
            taken = np.arange(rem.size)             # e_k = 0: nothing conflicts
        done.append(rem[taken])
        counts.append(int(taken.size))
        rem = np.delete(rem, taken)
    done.append(rem)
    counts.append(int(rem.size))
    order = (orig[np.concatenate(done)] + 1).astype(np.int32)
    return (order, np.asarray(counts, dtype=np.int32)) if levels else order


def vecchia_order_device(locs, device=0, levels=False):
    """`vecchia_order` on the device (cocons_vecchia_order): the same bits.  levels=True: (order, counts) with
    counts = [level 0, levels 1 .. K, the rest]."""
    L = _lib.load()
    locs = _f(locs)
    n = locs.shape[0]
    order = np.zeros(n, dtype=np.int32)
    counts = np.zeros(_ORDER_LEVELS + 3, dtype=np.int32)
    _lib.check(L.cocons_vecchia_order(n, _p(locs), int(device), _ip(order), _ip(counts)), "cocons_vecchia_order")
    return (order, counts[1:1 + counts[0]].copy()) if levels else order


def vecchia_group(nn, max_rows=64, stats=False):
    """The greedy grouping of the rows of the neighbour table `nn` (cocons_vecchia_group; Guinness 2018): n
    int32 block ids, 0-based, numbered by their smallest member.  Rows are visited in ascending order; for each neighbour j of
    row i, in the order the row lists them, the blocks of i and j are merged when the union u of their row sets S (members and
    all their neighbours) has u <= max_rows and u^2 < |S(A)|^2 + |S(B)|^2.  With `stats` also {"blocks", "rows": the sum of
    |S|, "pairs": what the grouped schedule evaluates, "pairs_ungrouped": what the ungrouped schedule evaluates on nn}.  The
    rule runs on the host; nothing here needs a device."""
    L = _lib.load()
    nn = np.asarray(nn)
    nn, m = _nn_table(nn, nn.shape[0])
    group = np.zeros(nn.shape[0], dtype=np.int32)
    out = (ctypes.c_longlong * 4)()
    _lib.check(L.cocons_vecchia_group(nn.shape[0], m, _ip(nn), int(max_rows), _ip(group), out), "cocons_vecchia_group")
    if stats:
        return group, {"blocks": int(out[0]), "rows": int(out[1]), "pairs": int(out[2]), "pairs_ungrouped": int(out[3])}
    return group


def _group_rounds(entry, nn, max_rows, max_rounds, stats, *device):
    L = _lib.load()
    nn = np.asarray(nn)
    nn, m = _nn_table(nn, nn.shape[0])
    group = np.zeros(nn.shape[0], dtype=np.int32)
    out = (ctypes.c_longlong * 5)()
    _lib.check(getattr(L, entry)(nn.shape[0], m, _ip(nn), int(max_rows), int(max_rounds), *device, _ip(group), out), entry)
    if stats:
        return group, {"blocks": int(out[0]), "rows": int(out[1]), "pairs": int(out[2]), "pairs_ungrouped": int(out[3]),
                       "rounds": int(out[4])}
    return group


def vecchia_group_rounds(nn, max_rows=64, max_rounds=0, stats=False):
    """The ROUND rule's grouping of the rows of `nn` (cocons_vecchia_group_rounds): n int32 block ids, 0-based,
    numbered by their smallest member.  Every round, each block proposes the neighbouring block whose merge saves the most
    (the gain |S(A)|^2 + |S(B)|^2 - |S(A) u S(B)|^2 under `vecchia_group`'s test, ties to the smaller id), and the proposals
    that are the best of both their blocks are merged; the rounds end when nobody proposes, or after `max_rounds` (0: 256).
    The partition is a function of the rows' neighbour sets and is not the greedy one.  `stats` as `vecchia_group`'s, with
    "rounds", the rounds that merged something.  On the host; nothing here needs a device."""
    return _group_rounds("cocons_vecchia_group_rounds", nn, max_rows, max_rounds, stats)


def vecchia_group_device(nn, max_rows=64, max_rounds=0, stats=False, device=0):
    """`vecchia_group_rounds` on the device (cocons_vecchia_group_device): the same labels and rounds, integer for integer."""
    return _group_rounds("cocons_vecchia_group_device", nn, max_rows, max_rounds, stats, int(device))


def vecchia_group_table(nn, group, m_out=None) -> np.ndarray:
    """The expanded table of ANY partition `group` of nn's rows (cocons_vecchia_group_table): row i names every earlier row of
    S(block(i)) -- its own neighbours and those of the block's other members --, n x m_out int32 in Fortran order, 1-based,
    ascending, zero padded; m_out None: the longest expanded row (at least 1).  The grouped model is the ordinary Vecchia
    model on this table."""
    L = _lib.load()
    nn = np.asarray(nn)
    nn, m = _nn_table(nn, nn.shape[0])
    n = nn.shape[0]
    group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(n))
    if m_out is None:
        m_out = L.cocons_vecchia_group_table(n, m, _ip(nn), _ip(group), 0, None)
        _lib.check(min(m_out, 0), "cocons_vecchia_group_table")
        m_out = max(m_out, 1)
    out = np.zeros((n, int(m_out)), dtype=np.int32, order="F")
    _lib.check(L.cocons_vecchia_group_table(n, m, _ip(nn), _ip(group), int(m_out), _ip(out)), "cocons_vecchia_group_table")
    return out


class CoconsVecchiaFit(_Handle):
    """Handle of a Vecchia fit (cocons_fit_create_vecchia): (locs, x_covariates, z, smooth.limits) and the neighbour table
    `nn` (n x m, 1-based indices of EARLIER rows, 0 = none; `vecchia_neighbours` makes one).  The rows' order is the Vecchia
    order.  No n x n buffer exists; the library refuses this handle everywhere but in the cores below."""

    @classmethod
    def from_knn(cls, locs, x_covariates, z, smooth_limits, m, device=-1):
        """The handle of the table `vecchia_neighbours_device(locs, m)`: the library searches it on the device and keeps it
        there (cocons_fit_create_vecchia_knn); every core below gives the bits of the handle made from that table."""
        self = cls.__new__(cls)
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        self.m = int(m)
        self._created(self._L.cocons_fit_create_vecchia_knn(self.n, self.p, self.r, _p(locs), _p(X), _p(z),
                                                            _p(self.smooth_limits), int(device), self.m),
                      "cocons_fit_create_vecchia_knn")
        return self

    @classmethod
    def from_groups_knn(cls, locs, x_covariates, z, smooth_limits, m, max_rows=64, max_rounds=0, device=-1):
        """The grouped handle made on the device (cocons_fit_create_vecchia_grouped_knn): the search of
        `from_knn`, the round rule of `vecchia_group_device`, the plan and the expanded table, none of which reaches the host.
        The handle of `vecchia_neighbours_device` -> `vecchia_group_rounds` -> `vecchia_group_table` -> the constructor ->
        `set_groups` on the same data, to the bit; `groups_export` reads the partition and the table back."""
        self = cls.__new__(cls)
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        self._created(self._L.cocons_fit_create_vecchia_grouped_knn(self.n, self.p, self.r, _p(locs), _p(X), _p(z),
                                                                    _p(self.smooth_limits), int(device), int(m), int(max_rows),
                                                                    int(max_rounds)), "cocons_fit_create_vecchia_grouped_knn")
        self.m = self.info()["m"]
        return self

    @classmethod
    def from_maxmin(cls, locs, x_covariates, z, smooth_limits, m, device=-1):
        """`from_knn` on the rows in the maxmin order of `vecchia_order_device(locs)`: the order is found on the device, the
        data is permuted on the host, and every core gives the bits of `from_knn` on the permuted arrays.  The handle's rows
        are the PERMUTED ones: `maxmin_order` (n int32, 1-based) says which of the caller's rows stands where, `to_maxmin`
        carries per-row arrays of the caller (B of whiten_core, iiderrors, W) into the handle's order and `from_maxmin_order`
        carries per-row outputs (whitened columns, simulated fields) back.  `from_maxmin_groups` is the grouped form."""
        return cls._from_maxmin(cls.from_knn, locs, x_covariates, z, smooth_limits, m, device=device)

    @classmethod
    def from_maxmin_groups(cls, locs, x_covariates, z, smooth_limits, m, max_rows=64, max_rounds=0, device=-1):
        """`from_maxmin` with `from_groups_knn` in the place of `from_knn`: the order, the search, the round rule, the plan
        and the expanded table all on the device; the rows are the permuted ones, as `from_maxmin`'s are.  (A method of its
        own: `from_maxmin`'s argument list is part of the layer's contract.)"""
        return cls._from_maxmin(cls.from_groups_knn, locs, x_covariates, z, smooth_limits, m, max_rows=max_rows,
                                max_rounds=max_rounds, device=device)

    @classmethod
    def _from_maxmin(cls, make, locs, x_covariates, z, smooth_limits, m, device=-1, **more):
        locs = _f(locs)
        order = vecchia_order_device(locs, device=max(int(device), 0))
        o = order.astype(np.int64) - 1
        X = _f(x_covariates)
        z = np.asarray(z, dtype=np.float64).reshape(locs.shape[0], -1)
        self = make(locs[o], X[o], z[o], smooth_limits, m, device=device, **more)
        self.maxmin_order = order
        return self

    @classmethod
    def from_corr_knn(cls, locs, x_covariates, z, smooth_limits, theta_list, m, m_cand=None, hops=2, device=-1):
        """The handle of the table `neighbours_corr(theta_list, m, m_cand, hops)` (cocons_fit_create_vecchia_corr_knn, DESIGN.md
        4af): the Euclidean search of width m_cand (default min(2 m, 63)), the records at theta and the re-ranking by model
        correlation all on the device; neither table reaches the host, and every core gives the bits of the handle made
        from the exported table.  `from_groups_corr_knn` is the grouped handle on such a table."""
        self = cls.__new__(cls)
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        self.m = int(m)
        mc = min(2 * self.m, 63) if m_cand is None else int(m_cand)
        T = theta_table(theta_list)
        self._created(self._L.cocons_fit_create_vecchia_corr_knn(self.n, self.p, self.r, _p(locs), _p(X), _p(z),
                                                                 _p(self.smooth_limits), int(device), _p(T), mc, int(hops),
                                                                 self.m), "cocons_fit_create_vecchia_corr_knn")
        return self

    @classmethod
    def from_maxmin_corr(cls, locs, x_covariates, z, smooth_limits, theta_list, m, m_cand=None, hops=2, device=-1):
        """`from_maxmin` with `from_corr_knn` in the place of `from_knn`: the maxmin order, then the correlation table of the
        permuted rows at theta; the rows are the permuted ones, as `from_maxmin`'s are."""
        def make(locs_, X_, z_, sl_, m_, device=-1):
            return cls.from_corr_knn(locs_, X_, z_, sl_, theta_list, m_, m_cand=m_cand, hops=hops, device=device)
        return cls._from_maxmin(make, locs, x_covariates, z, smooth_limits, m, device=device)

    def neighbours_corr(self, theta_list, m, m_cand=None, hops=2):
        """The Vecchia neighbours of the handle's observations by model correlation at theta (cocons_vecchia_neighbours_corr,
        DESIGN.md 4af): among the candidates -- the m_cand (default min(2 m, 63)) Euclidean-nearest predecessors and, with
        hops = 2, theirs -- the m with the largest correlation under Sigma(theta), largest first: n x m int32 in Fortran
        order, 1-based, zero-padded.  `vecchia_neighbours_corr` restates the rule on the host.  The handle's own table is
        neither read nor changed.  CholeskyError(i): row i has a candidate whose correlation is not finite."""
        m = int(m)
        mc = min(2 * m, 63) if m_cand is None else int(m_cand)
        T = theta_table(theta_list)
        nn = np.zeros((self.n, m), dtype=np.int32, order="F")
        _lib.check(self._L.cocons_vecchia_neighbours_corr(self._h, _p(T), mc, int(hops), m, _ip(nn)),
                   "cocons_vecchia_neighbours_corr")
        return nn

    def neighbours_corr_pred(self, theta_list, locs_pred, x_covariates_pred, m, m_cand=None, hops=2):
        """The neighbours of new locations by model correlation at theta (cocons_vecchia_neighbours_corr_pred):
        among the candidates -- the m_cand (default min(2 m, 63)) nearest observations and, with hops = 2, the m_cand
        nearest observations of each of those -- the m with the largest correlation with the new location under the
        prediction's covariance, largest first: mp x m int32 in Fortran order, 1-based, zero-padded.
        `vecchia_neighbours_corr_pred` restates the rule on the host.  The first call builds the grid over the observations
        and, with hops = 2, their own kNN table of width m_cand, which the handle keeps (`info()["bytes"]` counts them).
        CholeskyError(q): row q has a candidate whose correlation is not finite."""
        m = int(m)
        mc = min(2 * m, 63) if m_cand is None else int(m_cand)
        T = theta_table(theta_list)
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        mp = lp.shape[0]
        nn = np.zeros((mp, m), dtype=np.int32, order="F")
        _lib.check(self._L.cocons_vecchia_neighbours_corr_pred(self._h, _p(T), mp, _p(lp), _p(Xp), mc, int(hops), m, _ip(nn)),
                   "cocons_vecchia_neighbours_corr_pred")
        return nn

    @classmethod
    def from_groups_corr_knn(cls, locs, x_covariates, z, smooth_limits, theta_list, m, m_cand=None, hops=2, max_rows=64,
                             max_rounds=0, device=-1):
        """`from_groups_knn` on the table `neighbours_corr(theta_list, m, m_cand, hops)` in the place of the Euclidean one
        (cocons_fit_create_vecchia_grouped_corr_knn): search, records at theta, re-ranking, round rule, plan
        and expanded table on the device, none of which reaches the host.  The handle of `neighbours_corr` ->
        `vecchia_group_rounds` -> `vecchia_group_table` -> the constructor -> `set_groups` on the same data, to the bit."""
        self = cls.__new__(cls)
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        m = int(m)
        mc = min(2 * m, 63) if m_cand is None else int(m_cand)
        T = theta_table(theta_list)
        self._created(self._L.cocons_fit_create_vecchia_grouped_corr_knn(self.n, self.p, self.r, _p(locs), _p(X), _p(z),
                                                                         _p(self.smooth_limits), int(device), _p(T), mc,
                                                                         int(hops), m, int(max_rows), int(max_rounds)),
                      "cocons_fit_create_vecchia_grouped_corr_knn")
        self.m = self.info()["m"]
        return self

    @classmethod
    def from_maxmin_groups_corr(cls, locs, x_covariates, z, smooth_limits, theta_list, m, m_cand=None, hops=2, max_rows=64,
                                max_rounds=0, device=-1):
        """`from_maxmin` with `from_groups_corr_knn` in the place of `from_knn`: the maxmin order, then the grouped handle
        on the correlation table of the permuted rows at theta; the rows are the permuted ones, as `from_maxmin`'s are."""
        def make(locs_, X_, z_, sl_, m_, device=-1):
            return cls.from_groups_corr_knn(locs_, X_, z_, sl_, theta_list, m_, m_cand=m_cand, hops=hops, max_rows=max_rows,
                                            max_rounds=max_rounds, device=device)
        return cls._from_maxmin(make, locs, x_covariates, z, smooth_limits, m, device=device)

    @classmethod
    def from_groups(cls, locs, x_covariates, z, smooth_limits, nn, max_rows=64, device=-1):
        """The handle of the grouped model of the table `nn` (cocons_fit_create_vecchia_grouped): the greedy
        groups of `vecchia_group(nn, max_rows)`, the handle of `vecchia_group_table(nn, groups)` and `set_groups(groups)` in
        one call.  Every core serves the model of the expanded table; `neg2loglik_core(theta, grouped=True)` and
        `whiten_grouped_core` run the grouped schedule."""
        self = cls.__new__(cls)
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        nn, m = _nn_table(nn, self.n)
        self._created(self._L.cocons_fit_create_vecchia_grouped(self.n, self.p, self.r, _p(locs), _p(X), _p(z),
                                                                _p(self.smooth_limits), int(device), m, _ip(nn),
                                                                int(max_rows)), "cocons_fit_create_vecchia_grouped")
        self.m = self.info()["m"]
        return self

    def set_groups(self, group):
        """Attach the plan of the partition `group` (n block labels) to the handle (cocons_vecchia_set_groups).  The handle's
        table must be closed under it -- `vecchia_group_table` makes such a table --; a second call replaces the plan.
        Returns {"blocks", "maxrows", "rows", "pairs", "bytes"} of the plan."""
        group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(self.n))
        _lib.check(self._L.cocons_vecchia_set_groups(self._h, _ip(group)), "cocons_vecchia_set_groups")
        return self.groups_info()

    def groups_info(self):
        out = (ctypes.c_longlong * 5)()
        _lib.check(self._L.cocons_vecchia_groups_info(self._h, out), "cocons_vecchia_groups_info")
        return {"blocks": int(out[0]), "maxrows": int(out[1]), "rows": int(out[2]), "pairs": int(out[3]), "bytes": int(out[4])}

    def groups_export(self, table=True):
        """(block, nn): the 0-based block of every row in the plan's numbering and, with `table`, the handle's table (n x m
        int32 in Fortran order, 1-based, ascending, 0 = none) -- cocons_vecchia_groups_export"""
        block = np.zeros(self.n, dtype=np.int32)
        nn = np.zeros((self.n, self.info()["m"]), dtype=np.int32, order="F") if table else None
        _lib.check(self._L.cocons_vecchia_groups_export(self._h, _ip(block), None if nn is None else _ip(nn)),
                   "cocons_vecchia_groups_export")
        return (block, nn) if table else block

    def to_maxmin(self, rows):
        """A per-row array in the caller's order (n or n x c) in the handle's order (`from_maxmin`)"""
        return np.asarray(rows)[self.maxmin_order.astype(np.int64) - 1]

    def from_maxmin_order(self, rows):
        """A per-row array in the handle's order (n or n x c) in the caller's order: the inverse of `to_maxmin`"""
        rows = np.asarray(rows)
        out = np.empty_like(rows)
        out[self.maxmin_order.astype(np.int64) - 1] = rows
        return out

    def __init__(self, locs, x_covariates, z, smooth_limits, nn, device=-1):
        locs, X, z = self._adopt(locs, x_covariates, z, smooth_limits)
        nn, self.m = _nn_table(nn, self.n)
        self._created(self._L.cocons_fit_create_vecchia(self.n, self.p, self.r, _p(locs), _p(X), _p(z), _p(self.smooth_limits),
                                                        int(device), self.m, _ip(nn)), "cocons_fit_create_vecchia")

    def neg2loglik_core(self, theta_list, grouped=False):
        """(value, parts): parts[0] = sum_i log d_i, parts[1 + k] = sum_i y_ik^2, value = sum_k [n log 2 pi + 2 parts[0] +
        parts[1 + k]].  CholeskyError(i): the block of row i has a conditional variance that is not positive.  `grouped`:
        on the plan of `set_groups`, one factorisation per block (cocons_neg2loglik_vecchia_grouped) -- the same bits."""
        T, mean = _table_mean(theta_list)
        val = ctypes.c_double(0.0)
        parts = np.zeros(1 + self.r)
        entry = "cocons_neg2loglik_vecchia_grouped" if grouped else "cocons_neg2loglik_vecchia"
        _lib.check(getattr(self._L, entry)(self._h, _p(T), _p(mean), ctypes.byref(val), _p(parts)), entry)
        return val.value, parts

    def neg2loglik_grad_core(self, theta_list, B=None, grouped=False):
        """(value, parts, grad_table, grad_quad, grad_mean) of cocons_neg2loglik_grad_vecchia: value and parts are
        neg2loglik_core's to the bit, grad_table the 6 x p table of the whole value in the conventions of the dense
        gradient, grad_quad the quadratic forms' share of it (the log-determinant's is grad_table - grad_quad), grad_mean p
        doubles.  With B (n x c, the caller's order) the columns are used as given -- the forms with the mean profiled out
        --, parts has 1 + c entries and grad_mean is None.  `grouped`: on the plan of `set_groups`, one factorisation per block
        and every pair of a block once (cocons_neg2loglik_grad_vecchia_grouped) -- value and parts to the bit, the gradient of
        the same model to rounding."""
        T = theta_table(theta_list)
        val = ctypes.c_double(0.0)
        gt, gq = np.zeros((6, self.p)), np.zeros((6, self.p))
        entry = "cocons_neg2loglik_grad_vecchia_grouped" if grouped else "cocons_neg2loglik_grad_vecchia"
        call = getattr(self._L, entry)
        if B is None:
            mean = np.ascontiguousarray(np.asarray(theta_list["mean"], dtype=np.float64))
            parts, gm = np.zeros(1 + self.r), np.zeros(self.p)
            st = call(self._h, _p(T), _p(mean), 0, None, ctypes.byref(val), _p(parts), _p(gt), _p(gq), _p(gm))
        else:
            B = _f(np.asarray(B, dtype=np.float64).reshape(self.n, -1))
            parts, gm = np.zeros(1 + B.shape[1]), None
            st = call(self._h, _p(T), None, int(B.shape[1]), _p(B), ctypes.byref(val), _p(parts), _p(gt), _p(gq), None)
        _lib.check(st, entry)
        return val.value, parts, gt, gq, gm

    def fisher_core(self, theta_list, dirs, grouped=False):
        """Expected information of the Vecchia likelihood at `theta_list` (cocons_fisher_vecchia), `dirs` as for
        `CoconsFit.fisher_core` (ndir x 6 x p or ndir x 6p).  Returns (info ndir x ndir, info_mean p x p): the sums over the
        n blocks of the block's information minus that of its neighbours alone, and r (U X)'(U X) with U the whitening.
        Both are Gram matrices, symmetric to the bit; with every predecessor in the table they are the dense ones.  `grouped`:
        on the plan of `set_groups`, one factorisation per block and every pair of a block once per walk
        (cocons_fisher_vecchia_grouped) -- the information of the same model to rounding."""
        entry = "cocons_fisher_vecchia_grouped" if grouped else "cocons_fisher_vecchia"
        T = theta_table(theta_list)
        D = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 6 * self.p))
        nd = D.shape[0]
        info = np.zeros((nd, nd))
        info_mean = np.zeros((self.p, self.p))
        _lib.check(getattr(self._L, entry)(self._h, _p(T), nd, _p(D), _p(info), _p(info_mean)), entry)
        return info, info_mean

    def _whiten(self, theta_list, B, entry):
        T = theta_table(theta_list)
        B = _f(np.asarray(B, dtype=np.float64).reshape(self.n, -1))
        out, logd = np.zeros(B.shape, order="F"), np.zeros(self.n)
        _lib.check(getattr(self._L, entry)(self._h, _p(T), int(B.shape[1]), _p(B), _p(out), _p(logd)), entry)
        return out, logd

    def whiten_core(self, theta_list, B):
        """(U B, log d) for the columns of B (n x c, the caller's order): U'U is the approximation's Sigma^-1."""
        return self._whiten(theta_list, B, "cocons_vecchia_whiten")

    def whiten_grouped_core(self, theta_list, B):
        """`whiten_core` on the plan of `set_groups`, one factorisation per block (cocons_vecchia_whiten_grouped): the same
        bits.  (A method of its own: `whiten_core`'s signature is part of the layer's contract.)"""
        return self._whiten(theta_list, B, "cocons_vecchia_whiten_grouped")

    def predict_core(self, theta_list, locs_pred, x_covariates_pred, nn_pred, z_col=0):
        """Local kriging: (stochastic, quadform) of cocons_vecchia_predict for the neighbour table nn_pred (mp x m_pred,
        1-based indices into the observations, 0 = none; `vecchia_neighbours_pred` makes one)."""
        T, mean = _table_mean(theta_list)
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        mp = lp.shape[0]
        nnp, m_pred = _nn_table(nn_pred, mp)
        st, qf = np.zeros(mp), np.zeros(mp)
        _lib.check(self._L.cocons_vecchia_predict(self._h, _p(T), _p(mean), int(z_col), mp, _p(lp), _p(Xp), m_pred, _ip(nnp),
                                                  _p(st), _p(qf)), "cocons_vecchia_predict")
        return st, qf

    def predict_knn_core(self, theta_list, locs_pred, x_covariates_pred, m_pred, z_col=0):
        """`predict_core` with the table `vecchia_neighbours_pred_device(locs, locs_pred, m_pred)`, to the bit
        (cocons_vecchia_predict_knn): the neighbours are found on the device chunk by chunk.  The first call builds the grid
        over the observations, which the handle keeps (`info()["bytes"]` counts it)."""
        T, mean = _table_mean(theta_list)
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        mp = lp.shape[0]
        st, qf = np.zeros(mp), np.zeros(mp)
        _lib.check(self._L.cocons_vecchia_predict_knn(self._h, _p(T), _p(mean), int(z_col), mp, _p(lp), _p(Xp), int(m_pred),
                                                      _p(st), _p(qf)), "cocons_vecchia_predict_knn")
        return st, qf

    def predict_corr_knn_core(self, theta_list, locs_pred, x_covariates_pred, m_pred, m_cand=None, hops=2, z_col=0):
        """`predict_core` with the table `neighbours_corr_pred(theta_list, locs_pred, x_covariates_pred, m_pred, m_cand,
        hops)`, to the bit (cocons_vecchia_predict_corr_knn): every chunk's neighbours are found and ranked by
        model correlation on the device, and no table goes up or down.  What the handle keeps is `neighbours_corr_pred`'s."""
        T, mean = _table_mean(theta_list)
        lp, Xp = _f(locs_pred), _f(x_covariates_pred)
        mp, m_pred = lp.shape[0], int(m_pred)
        mc = min(2 * m_pred, 63) if m_cand is None else int(m_cand)
        st, qf = np.zeros(mp), np.zeros(mp)
        _lib.check(self._L.cocons_vecchia_predict_corr_knn(self._h, _p(T), _p(mean), int(z_col), mp, _p(lp), _p(Xp), mc,
                                                           int(hops), m_pred, _p(st), _p(qf)),
                   "cocons_vecchia_predict_corr_knn")
        return st, qf

    def _unwhiten(self, theta_list, W, entry):
        T = theta_table(theta_list)
        W = _f(np.asarray(W, dtype=np.float64).reshape(self.n, -1))
        out = np.zeros(W.shape, order="F")
        _lib.check(getattr(self._L, entry)(self._h, _p(T), int(W.shape[1]), _p(W), _p(out)), entry)
        return out

    def unwhiten_core(self, theta_list, W):
        """U^-1 W for the columns of W (n x c, the caller's order): the inverse of `whiten_core` for the same theta
        (cocons_vecchia_unwhiten).  With N(0, 1) columns the result has the Vecchia model's covariance."""
        return self._unwhiten(theta_list, W, "cocons_vecchia_unwhiten")

    def unwhiten_grouped_core(self, theta_list, W):
        """`unwhiten_core` with the rows' coefficients from one factorisation per block of the plan of `set_groups`
        (cocons_vecchia_unwhiten_grouped): the same bits.  (A method of its own, as `whiten_grouped_core`.)"""
        return self._unwhiten(theta_list, W, "cocons_vecchia_unwhiten_grouped")

    def _sim(self, theta_list, iiderrors, n_fixed, z_col, entry):
        rows = self.n - int(n_fixed)
        E = _f(np.asarray(iiderrors, dtype=np.float64).reshape(max(rows, 1), -1))
        T, mean = _table_mean(theta_list)
        out = np.zeros(E.shape, order="F")
        _lib.check(getattr(self._L, entry)(self._h, _p(T), _p(mean), int(n_fixed), int(z_col), int(E.shape[1]), _p(E), _p(out)),
                   entry)
        return out

    def sim_core(self, theta_list, iiderrors, n_fixed=0, z_col=0):
        """cocons_sim_vecchia.  n_fixed = 0: X mean + U^-1 E, n x nsim.  1 <= n_fixed < n: the first n_fixed rows are data
        (z[:, z_col] - X mean) and the rows behind them run the recursion; E and the result are (n - n_fixed) x nsim -- the
        joint conditional mean at the later rows for E = 0, a conditional draw for N(0, 1) numbers."""
        return self._sim(theta_list, iiderrors, n_fixed, z_col, "cocons_sim_vecchia")

    def sim_grouped_core(self, theta_list, iiderrors, n_fixed=0, z_col=0):
        """`sim_core` with the coefficients of the rows n_fixed .. n - 1 from one factorisation per block of the plan of
        `set_groups` (cocons_sim_vecchia_grouped): the same bits."""
        return self._sim(theta_list, iiderrors, n_fixed, z_col, "cocons_sim_vecchia_grouped")

    def schedule(self, n_fixed=0):
        """The level schedule of (table, n_fixed) that `unwhiten_core` and `sim_core` run on (cocons_vecchia_schedule):
        {"levels": n int32 (0: a fixed row), "depth", "widest": rows of the largest level, "launches": of one solve under the
        current COCONS_VECCHIA_SIM_FUSE, "bytes": device bytes of the schedule and of a solve's coefficients}"""
        levels = np.zeros(self.n, dtype=np.int32)
        out = (ctypes.c_longlong * 4)()
        _lib.check(self._L.cocons_vecchia_schedule(self._h, int(n_fixed), _ip(levels), out), "cocons_vecchia_schedule")
        return {"levels": levels, "depth": int(out[0]), "widest": int(out[1]), "launches": int(out[2]), "bytes": int(out[3])}

    def transpose(self):
        """The transposed lists of the handle's table (cocons_vecchia_transpose): {"ptr": n + 1 int32 0-based
        offsets, "rows": the 1-based rows that name column j at rows[ptr[j]:ptr[j + 1]], ascending, "entries", "longest":
        the longest list, "bytes": device bytes of the lists, "unnamed": columns nobody names}.  Built by the first call that
        needs them and kept by the handle (`info()["bytes"]` counts them)."""
        out = (ctypes.c_longlong * 4)()
        _lib.check(self._L.cocons_vecchia_transpose(self._h, None, None, out), "cocons_vecchia_transpose")
        ptr = np.zeros(self.n + 1, dtype=np.int32)
        rows = np.zeros(int(out[0]), dtype=np.int32)
        _lib.check(self._L.cocons_vecchia_transpose(self._h, _ip(ptr), _ip(rows) if rows.size else None, out),
                   "cocons_vecchia_transpose")
        return {"ptr": ptr, "rows": rows, "entries": int(out[0]), "longest": int(out[1]), "bytes": int(out[2]),
                "unnamed": int(out[3])}

    def _whiten_t(self, theta_list, W, entry):
        T = theta_table(theta_list)
        W = _f(np.asarray(W, dtype=np.float64).reshape(self.n, -1))
        out, qd = np.zeros(W.shape, order="F"), np.zeros(self.n)
        _lib.check(getattr(self._L, entry)(self._h, _p(T), int(W.shape[1]), _p(W), _p(out), _p(qd)), entry)
        return out, qd

    def whiten_t_core(self, theta_list, W):
        """(U'W, diag(U'U)) for the columns of W (n x c, the caller's order): the transpose of `whiten_core`'s U, applied
        through the transposed lists in a fixed order (cocons_vecchia_whiten_t).  A column's result does not depend on c."""
        return self._whiten_t(theta_list, W, "cocons_vecchia_whiten_t")

    def whiten_t_grouped_core(self, theta_list, W):
        """`whiten_t_core` with the rows' coefficients from one factorisation per block of the plan of `set_groups`
        (cocons_vecchia_whiten_t_grouped): the same bits."""
        return self._whiten_t(theta_list, W, "cocons_vecchia_whiten_t_grouped")

    def unwhiten_t_core(self, theta_list, W, grouped=False):
        """U^-T W for the columns of W (n x c, the caller's order): the inverse of `whiten_t_core` for the same theta, by the
        descending level solve over the transposed lists (cocons_vecchia_unwhiten_t).  A column's result does
        not depend on c.  `grouped`: the coefficients from one factorisation per block of the plan of `set_groups` -- the
        same bits."""
        T = theta_table(theta_list)
        W = _f(np.asarray(W, dtype=np.float64).reshape(self.n, -1))
        out = np.zeros(W.shape, order="F")
        _lib.check(self._L.cocons_vecchia_unwhiten_t(self._h, _p(T), int(bool(grouped)), int(W.shape[1]), _p(W), _p(out)),
                   "cocons_vecchia_unwhiten_t")
        return out

    def cov_mult_core(self, theta_list, B, n_fixed=0, grouped=False):
        """U_pp^-1 U_pp^-T B for the columns of B ((n - n_fixed) x c), U_pp the block of U on the rows >= n_fixed
        (cocons_vecchia_cov_mult).  n_fixed = 0: the Vecchia model's own covariance (U'U)^-1 times B; on a joint handle over
        (observations, then new locations) with n_fixed = the observations: Cov(new | data) B."""
        T = theta_table(theta_list)
        B = _f(np.asarray(B, dtype=np.float64).reshape(max(self.n - int(n_fixed), 1), -1))
        out = np.zeros(B.shape, order="F")
        _lib.check(self._L.cocons_vecchia_cov_mult(self._h, _p(T), int(bool(grouped)), int(n_fixed), int(B.shape[1]), _p(B),
                                                   _p(out)), "cocons_vecchia_cov_mult")
        return out

    def cov_cols_core(self, theta_list, idx, n_fixed=0, grouped=False):
        """The columns `idx` (1-based rows of the handle, each > n_fixed; repeats allowed) of U_pp^-1 U_pp^-T,
        (n - n_fixed) x len(idx): `cov_mult_core` on unit columns made on the device, to the bit (cocons_vecchia_cov_cols)."""
        T = theta_table(theta_list)
        idx = np.ascontiguousarray(np.asarray(idx).ravel(), dtype=np.int32)
        out = np.zeros((max(self.n - int(n_fixed), 1), max(idx.size, 1)), order="F")
        _lib.check(self._L.cocons_vecchia_cov_cols(self._h, _p(T), int(bool(grouped)), int(n_fixed), int(idx.size), _ip(idx),
                                                   _p(out)), "cocons_vecchia_cov_cols")
        return out

    def schedule_t(self, n_fixed=0):
        """The transposed level schedule of (table, n_fixed) that `unwhiten_t_core` and the covariance entries run on
        (cocons_vecchia_schedule_t): {"levels": n int32 (0: a fixed row), "depth", "widest": rows of the largest level,
        "launches": of one solve of one column under the current COCONS_VECCHIA_SOLVE_T_FUSE, "bytes": device bytes of the
        schedule}"""
        levels = np.zeros(self.n, dtype=np.int32)
        out = (ctypes.c_longlong * 4)()
        _lib.check(self._L.cocons_vecchia_schedule_t(self._h, int(n_fixed), _ip(levels), out), "cocons_vecchia_schedule_t")
        return {"levels": levels, "depth": int(out[0]), "widest": int(out[1]), "launches": int(out[2]), "bytes": int(out[3])}

    def cv_core(self, theta_list, fold=None, stats=False, grouped=False):
        """Cross-validated predictions of the Vecchia model from Q = U'U (cocons_cv_vecchia).  `fold`: n integer labels in
        [0, nfold), every fold of at most 128 observations (None: leave-one-out).  Returns (resid n x r, var n) as
        `CoconsFit.cv_core`; with `stats` also {"singles", "folds", "entries", "bytes": device bytes of the call}.  `grouped`:
        the coefficients from one factorisation per block of the plan of `set_groups` (cocons_cv_vecchia_grouped, DESIGN.md
        4ab) -- the same bits."""
        entry = "cocons_cv_vecchia_grouped" if grouped else "cocons_cv_vecchia"
        T, mean = _table_mean(theta_list)
        resid = np.zeros((self.n, self.r), order="F")
        var = np.zeros(self.n)
        nfold, lab = (0, None) if fold is None else _fold_labels(fold, self.n)
        st = (ctypes.c_longlong * 4)()
        _lib.check(getattr(self._L, entry)(self._h, _p(T), _p(mean), nfold, None if lab is None else _ip(lab), _p(resid), _p(var),
                                           st), entry)
        if stats:
            return resid, var, {"singles": int(st[0]), "folds": int(st[1]), "entries": int(st[2]), "bytes": int(st[3])}
        return resid, var

    def info(self):
        """{"n", "m", "bytes": device bytes the handle holds, "rows": rows per chunk of predict_core}"""
        out = (ctypes.c_longlong * 4)()
        _lib.check(self._L.cocons_vecchia_info(self._h, out), "cocons_vecchia_info")
        return {"n": int(out[0]), "m": int(out[1]), "bytes": int(out[2]), "rows": int(out[3])}


def GetNeg2loglikelihoodVecchia(theta, par_pos, nn, locs, x_covariates, smooth_limits, z, n, lam, safe=True, fit=None,
                                grouped=False):
    """GetNeg2loglikelihood (R/neg2loglikelihood.R:183-222) with the Vecchia approximation of the likelihood for the neighbour
    table `nn`; `fit` (optional) a CoconsVecchiaFit built once from the same data and table.  `grouped`: the grouped model of
    `nn` on the grouped schedule (`fit` then a handle of `CoconsVecchiaFit.from_groups` or one with a plan)."""
    return _objective(theta, par_pos, lam, smooth_limits, safe, _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped),
                      lambda f, tl: f.neg2loglik_core(tl, grouped=grouped)[0], n)


def _vecchia_gls(f, tl, z, x_betas, grouped=False):
    """One whitening of [z | x_betas]: (sum log d, W = Xb' U'U Xb, the r quadratic forms z_k' P z_k with
    P = U'U - U'U Xb W^-1 Xb' U'U)."""
    z = np.asarray(z, dtype=np.float64).reshape(f.n, -1)
    xb = np.asarray(x_betas, dtype=np.float64).reshape(f.n, -1)
    UB, logd = (f.whiten_grouped_core if grouped else f.whiten_core)(tl, np.hstack([z, xb]))
    Uz, UX = UB[:, :z.shape[1]], UB[:, z.shape[1]:]
    W = UX.T @ UX
    g = UX.T @ Uz
    quad = np.sum(Uz * Uz, axis=0) - np.sum(g * np.linalg.solve(W, g), axis=0)
    return float(np.sum(logd)), W, quad


def GetNeg2loglikelihoodVecchiaProfile(theta, par_pos, nn, locs, x_covariates, smooth_limits, z, n, x_betas, lam,
                                       safe=True, fit=None, grouped=False):
    """R/neg2loglikelihood.R:127-165 with Sigma^-1 replaced by U'U; `grouped` as in GetNeg2loglikelihoodVecchia."""
    def core(f, tl):
        logdet, _, quad = _vecchia_gls(f, tl, z, x_betas, grouped)
        return float(np.sum(n * np.log(2 * np.pi) + 2 * logdet + quad))

    return _objective(theta, par_pos, lam, smooth_limits, safe, _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped),
                      core, n)


def GetNeg2loglikelihoodVecchiaREML(theta, par_pos, nn, locs, x_covariates, x_betas, smooth_limits, z, n, lam,
                                    safe=True, fit=None, grouped=False):
    """R/neg2loglikelihood.R:241-291 with Sigma^-1 replaced by U'U (x_betas is accepted and, as in the reference, unused:
    the restricted likelihood projects out x_covariates); `grouped` as in GetNeg2loglikelihoodVecchia."""
    X = np.asarray(x_covariates, dtype=np.float64)
    rank = int(np.linalg.matrix_rank(X))                    # qr(x)$rank, :270

    def core(f, tl):
        logdet, W, quad = _vecchia_gls(f, tl, z, X, grouped)
        logdet_w = float(np.sum(np.log(np.diag(np.linalg.cholesky(W)))))
        return float(np.sum((n - rank) * np.log(2 * np.pi) + 2 * logdet + 2 * logdet_w + quad))

    return _objective(theta, par_pos, lam, smooth_limits, safe, _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped),
                      core, n - rank)


def GetNeg2loglikelihoodVecchia_grad(theta, par_pos, nn, locs, x_covariates, smooth_limits, z, n, lam, safe=True, fit=None,
                                     grouped=False):
    """`GetNeg2loglikelihoodVecchia` and its gradient over the optimiser's vector `theta` in one call: (value, gradient).
    The value is that function's to the bit; the gradient is cocons_neg2loglik_grad_vecchia's plus the penalty's, carried
    through getModelLists(type="diff") as GetNeg2loglikelihood_grad does.  A failing block gives (1e6, zeros) under `safe`.
    `grouped`: the grouped model of `nn` with value and gradient on the grouped schedule, as in
    GetNeg2loglikelihoodVecchia."""
    def core(f, tl):
        val, _, gt, _, gm = f.neg2loglik_grad_core(tl, grouped=grouped)
        return val, (gt,), gm

    return _objective(theta, par_pos, lam, smooth_limits, safe, _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped),
                      core, n, grad=True)


def getFisher_vecchia(par, par_pos, locs, x_covariates, smooth_limits, z, n, nn, fit=None, grouped=False):
    """The P x P expected information of the Vecchia fit for the neighbour table `nn` in the optimiser's coordinates, rows
    and columns in `par`'s order, from ONE pass over the n blocks (cocons_fisher_vecchia): the expectation under the model of
    the Hessian of half of `GetNeg2loglikelihoodVecchia` without its penalty -- what GpGp returns as `info`.  It goes
    through `fisher_jacobian` as `getFisher_dense` does: the covariance block from the Jacobian's rows as directions, then
    J_m info_mean J_m' for the mean; the block between them is 0.  A Gram matrix, so solve() of it gives non-negative
    variances.  It is not the observed Hessian and not the Godambe (sandwich) information of the composite likelihood.
    A failing block raises CholeskyError.  `grouped`: the grouped model of `nn` with the information on the grouped schedule
    (cocons_fisher_vecchia_grouped), as in GetNeg2loglikelihoodVecchia_grad."""
    return _fisher_in_par(par, par_pos, _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped), grouped=grouped)


def _vecchia_gls_resid(f, tl, z, x_betas, grouped=False):
    """One whitening of [z | x_betas]: (W = Xb' U'U Xb, the residual columns z_k - Xb beta_k at the GLS estimate)."""
    z = np.asarray(z, dtype=np.float64).reshape(f.n, -1)
    xb = np.asarray(x_betas, dtype=np.float64).reshape(f.n, -1)
    UB, _ = (f.whiten_grouped_core if grouped else f.whiten_core)(tl, np.hstack([z, xb]))
    Uz, UX = UB[:, :z.shape[1]], UB[:, z.shape[1]:]
    W = UX.T @ UX
    return W, z - xb @ np.linalg.solve(W, UX.T @ Uz)


def GetNeg2loglikelihoodVecchiaProfile_grad(theta, par_pos, nn, locs, x_covariates, smooth_limits, z, n, x_betas, lam,
                                            safe=True, fit=None, grouped=False):
    """`GetNeg2loglikelihoodVecchiaProfile` and its gradient over the optimiser's vector: (value, gradient).  One whitening
    gives beta-hat; the gradient entry then runs on the columns z_k - Xb beta-hat_k.  By the envelope theorem the gradient
    at fixed beta-hat is the gradient of the profiled value (the mean is profiled out: `par_pos["mean"]` holds no free entry).
    `grouped` as in GetNeg2loglikelihoodVecchia_grad; the whitening of the GLS step runs on the grouped schedule too."""
    def core(f, tl):
        _, E = _vecchia_gls_resid(f, tl, z, x_betas, grouped)
        val, _, gt, _, _ = f.neg2loglik_grad_core(tl, B=E, grouped=grouped)
        return val, (gt,), None

    return _objective(theta, par_pos, lam, smooth_limits, safe, _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped),
                      core, n, grad=True)


def GetNeg2loglikelihoodVecchiaREML_grad(theta, par_pos, nn, locs, x_covariates, x_betas, smooth_limits, z, n, lam,
                                         safe=True, fit=None, grouped=False):
    """`GetNeg2loglikelihoodVecchiaREML` and its gradient over the optimiser's vector: (value, gradient).  Beside the
    residual columns the restricted likelihood has log|X' U'U X|, whose derivative is sum_j d||U v_j||^2 at fixed
    V = X chol(X' U'U X)^-T: the gradient entry runs on B = [residual columns | sqrt(r) V]; the log-determinant's share
    (grad_theta - grad_quad) is scaled from B's columns to the r realisations, the quadratic forms' share taken as it is.
    x_betas is accepted and unused, as there.  A rank-deficient x_covariates is refused (ValueError).  `grouped` as in
    GetNeg2loglikelihoodVecchiaProfile_grad."""
    X = np.asarray(x_covariates, dtype=np.float64)
    rank = int(np.linalg.matrix_rank(X))
    if rank < X.shape[1]:
        raise ValueError("GetNeg2loglikelihoodVecchiaREML_grad: x_covariates has rank %d < %d columns "
                         "(X' U'U X has no Cholesky factor)" % (rank, X.shape[1]))

    def core(f, tl):
        r = f.r
        W, E = _vecchia_gls_resid(f, tl, z, X, grouped)
        Lw = np.linalg.cholesky(W)
        V = np.linalg.solve(Lw, X.T).T
        _, parts, gt, gq, _ = f.neg2loglik_grad_core(tl, B=np.hstack([E, np.sqrt(r) * V]), grouped=grouped)
        logdet_w = float(np.sum(np.log(np.diag(Lw))))
        val = float(np.sum((n - rank) * np.log(2 * np.pi) + 2 * parts[0] + 2 * logdet_w + parts[1:1 + r]))
        return val, ((gt - gq) * (r / (r + X.shape[1])) + gq,), None

    return _objective(theta, par_pos, lam, smooth_limits, safe, _vecchia(fit, locs, x_covariates, z, smooth_limits, nn, grouped),
                      core, n - rank, grad=True)


def cocoPredict_vecchia(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, nn_pred, type="pred", fit=None):
    """cocoPredict (R/predict.R:136-183) by local kriging: every new location is predicted from the observations its row of
    nn_pred names.  `fit` (optional) a CoconsVecchiaFit over the same data (its own table is not used here); without one a
    handle with a one-column table is made for the call."""
    def one_column():
        return CoconsVecchiaFit(locs, X_std, z, smooth_limits, np.zeros((np.asarray(X_std).shape[0], 1), dtype=np.int32))

    with _borrowed(fit, one_column) as f:
        st, qf = f.predict_core(theta_list, newlocs, X_pred_std, nn_pred)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def cocoPredict_vecchia_knn(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, m_pred, type="pred", fit=None):
    """`cocoPredict_vecchia` without nn_pred: every new location is predicted from its m_pred nearest observations, found on
    the device (cocons_vecchia_predict_knn).  `fit` as there."""
    def one_column():
        # a handle for the data alone: prediction never reads the handle's own table, so an all-zero column (every
        # observation independent) stands in for one, as in cocoPredict_vecchia
        return CoconsVecchiaFit(locs, X_std, z, smooth_limits, np.zeros((np.asarray(X_std).shape[0], 1), dtype=np.int32))

    with _borrowed(fit, one_column) as f:
        st, qf = f.predict_knn_core(theta_list, newlocs, X_pred_std, m_pred)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def cocoPredict_vecchia_corr_knn(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, m_pred, m_cand=None, hops=2,
                                 type="pred", fit=None):
    """`cocoPredict_vecchia_knn` with every new location predicted from the m_pred observations most correlated with it
    under the model at theta, not its m_pred nearest (cocons_vecchia_predict_corr_knn): the fit made with
    `from_corr_knn` and the kriging then condition by the same criterion.  m_cand, hops as in
    `CoconsVecchiaFit.neighbours_corr_pred`; `fit` as there."""
    def one_column():
        # (see cocoPredict_vecchia_knn)
        return CoconsVecchiaFit(locs, X_std, z, smooth_limits, np.zeros((np.asarray(X_std).shape[0], 1), dtype=np.int32))

    with _borrowed(fit, one_column) as f:
        st, qf = f.predict_corr_knn_core(theta_list, newlocs, X_pred_std, m_pred, m_cand=m_cand, hops=hops)
    return _predict_outputs(theta_list, X_pred_std, st, qf, type)


def cocoSim_vecchia(theta_list, locs, X_std, smooth_limits, iiderrors, nn=None, m=None, fit=None):
    """Marginal branch of cocoSim (R/sim.R:147-172) for the Vecchia model: X mean + U^-1 E, n x nsim, E = `iiderrors` the
    n x nsim matrix of N(0, 1) draws, used as given.  The rows' order is the Vecchia order.  The table is `nn`, or with `m`
    the m nearest earlier rows found on the device (`CoconsVecchiaFit.from_knn`); `fit` (optional) a CoconsVecchiaFit over
    (locs, X_std) with the table to draw from.  With every predecessor in the table the fields are `cocoSim_dense`'s of
    type "diff"."""
    n = np.asarray(X_std).shape[0]
    if fit is None and (nn is None) == (m is None):
        raise ValueError("cocoSim_vecchia: give a neighbour table nn, a number of neighbours m, or a fit")

    def make():
        if nn is not None:
            return CoconsVecchiaFit(locs, X_std, np.zeros(n), smooth_limits, nn)
        return CoconsVecchiaFit.from_knn(locs, X_std, np.zeros(n), smooth_limits, m)

    with _borrowed(fit, make) as f, _chol_error():
        return f.sim_core(theta_list, np.asarray(iiderrors, dtype=np.float64).reshape(n, -1))


def cocoCV_vecchia(theta_list, locs, X_std, smooth_limits, z, nn=None, m=None, fold=None, fit=None):
    """Cross-validated predictions of the Vecchia model at `theta_list` from its precision U'U (cocons_cv_vecchia): no refit
    and no n x n matrix.  `fold`: one label of any kind per observation, every fold of at most 128 observations (None:
    leave-one-out).  The table is `nn`, or with `m` the m nearest earlier rows found on the device; `fit` (optional) a
    CoconsVecchiaFit over the same data.  Returns what `cocoCV_dense` returns; with every predecessor in the table, its
    numbers.  A failing block raises CholeskyError."""
    if fit is None and (nn is None) == (m is None):
        raise ValueError("cocoCV_vecchia: give a neighbour table nn, a number of neighbours m, or a fit")
    lab = None if fold is None else np.unique(np.asarray(fold).ravel(), return_inverse=True)[1]

    def make():
        if nn is not None:
            return CoconsVecchiaFit(locs, X_std, z, smooth_limits, nn)
        return CoconsVecchiaFit.from_knn(locs, X_std, z, smooth_limits, m)

    with _borrowed(fit, make) as f:
        return _cv_result(f, z, *f.cv_core(theta_list, lab))


def _grouped(who, fit, locs, X_std, z, smooth_limits, nn, m, max_rows):
    """The caller's grouped handle `fit`, or the handle `CoconsVecchiaFit.from_groups` makes of the table `nn` -- with `m` of
    the m nearest earlier rows found on the device -- for the length of the block."""
    if fit is None and (nn is None) == (m is None):
        raise ValueError("%s: give a neighbour table nn, a number of neighbours m, or a fit" % who)

    def make():
        table = nn if nn is not None else vecchia_neighbours_device(locs, m)
        return CoconsVecchiaFit.from_groups(locs, X_std, z, smooth_limits, table, max_rows=max_rows)

    return _borrowed(fit, make)


def cocoSim_vecchia_grouped(theta_list, locs, X_std, smooth_limits, iiderrors, nn=None, m=None, max_rows=64, fit=None):
    """`cocoSim_vecchia` for the grouped model of the table, the rows' coefficients from one factorisation per
    block (cocons_sim_vecchia_grouped): X mean + U^-1 E of the expanded table, n x nsim.  Without `fit` the handle
    is `CoconsVecchiaFit.from_groups` of `nn` (or of the `m` nearest earlier rows) with blocks of at most `max_rows` rows; `fit`
    (optional) a CoconsVecchiaFit with a plan of groups, on which this returns `cocoSim_vecchia(..., fit=fit)`'s bits."""
    n = np.asarray(X_std).shape[0]
    with _grouped("cocoSim_vecchia_grouped", fit, locs, X_std, np.zeros(n), smooth_limits, nn, m, max_rows) as f, _chol_error():
        return f.sim_grouped_core(theta_list, np.asarray(iiderrors, dtype=np.float64).reshape(n, -1))


def cocoCV_vecchia_grouped(theta_list, locs, X_std, smooth_limits, z, nn=None, m=None, fold=None, max_rows=64, fit=None):
    """`cocoCV_vecchia` for the grouped model of the table, the rows' coefficients from one factorisation per block
    (cocons_cv_vecchia_grouped).  The handle as in `cocoSim_vecchia_grouped`; on a `fit` with a plan of groups
    this returns `cocoCV_vecchia(..., fit=fit)`'s bits."""
    lab = None if fold is None else np.unique(np.asarray(fold).ravel(), return_inverse=True)[1]
    with _grouped("cocoCV_vecchia_grouped", fit, locs, X_std, z, smooth_limits, nn, m, max_rows) as f:
        return _cv_result(f, z, *f.cv_core(theta_list, lab, grouped=True))


def cocoSim_cond_vecchia(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, iiderrors, m, fit=None):
    """Conditional branch of cocoSim (sim.type = "cond") for the Vecchia model: the joint handle over (observations, then new
    locations) with the m nearest earlier rows of every row, found on the device -- a new location is conditioned on
    observations and on the new locations in front of it --, the observations fixed at z (its first column) and the
    recursion run over the new rows: mp x nsim, X_pred mean + x.  `iiderrors` (mp x nsim) = 0 gives the joint conditional mean
    of the model.  `fit` (optional): such a joint handle, made once."""
    X, Xp = np.asarray(X_std, dtype=np.float64), np.asarray(X_pred_std, dtype=np.float64)
    n, mp = X.shape[0], Xp.shape[0]

    def make():
        zz = np.asarray(z, dtype=np.float64).reshape(n, -1)
        return CoconsVecchiaFit.from_knn(np.vstack([np.asarray(locs, dtype=np.float64), np.asarray(newlocs, dtype=np.float64)]),
                                         np.vstack([X, Xp]), np.vstack([zz, np.zeros((mp, zz.shape[1]))]), smooth_limits, m)

    with _borrowed(fit, make) as f, _chol_error():
        return f.sim_core(theta_list, np.asarray(iiderrors, dtype=np.float64).reshape(mp, -1), n_fixed=n)


def cocoPredict_vecchia_joint(theta_list, locs, newlocs, X_std, X_pred_std, smooth_limits, z, m, cov_idx=None, fit=None):
    """Joint prediction of the Vecchia model at new locations that depend on each other: the joint handle of
    `cocoSim_cond_vecchia` over (observations, then new locations), the observations fixed at z (its first column).  Returns
    {"mean": the joint conditional mean, mp (`cocoSim_cond_vecchia` with zero errors, to the bit), "cov": the columns
    `cov_idx` (1-based new locations; None: all of them) of the predictive covariance Cov(new | data) = (U_pp' U_pp)^-1,
    mp x len(cov_idx) (cocons_vecchia_cov_cols)}.  `fit` (optional): such a joint handle, made once."""
    X, Xp = np.asarray(X_std, dtype=np.float64), np.asarray(X_pred_std, dtype=np.float64)
    n, mp = X.shape[0], Xp.shape[0]
    cols = np.arange(1, mp + 1) if cov_idx is None else np.asarray(cov_idx).ravel().astype(np.int64)
    if cols.size < 1 or cols.min() < 1 or cols.max() > mp:
        raise ValueError("cocoPredict_vecchia_joint: cov_idx must name new locations 1 .. %d" % mp)

    def make():
        zz = np.asarray(z, dtype=np.float64).reshape(n, -1)
        return CoconsVecchiaFit.from_knn(np.vstack([np.asarray(locs, dtype=np.float64), np.asarray(newlocs, dtype=np.float64)]),
                                         np.vstack([X, Xp]), np.vstack([zz, np.zeros((mp, zz.shape[1]))]), smooth_limits, m)

    with _borrowed(fit, make) as f, _chol_error():
        mean = f.sim_core(theta_list, np.zeros((mp, 1)), n_fixed=n)[:, 0]
        cov = f.cov_cols_core(theta_list, cols + n, n_fixed=n)
    return {"mean": mean, "cov": cov}
