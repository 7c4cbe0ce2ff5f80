"""Taper patterns from delta at the boundary, without a GPU: the headers declare cocons_taper_pattern,
cocons_fit_create_taper_delta, cocons_krige_taper_apply_delta, the three kind constants and cocons_debug_pattern_cells, the
library exports them and the ctypes binding carries them; every bad call is refused with -1 and a message naming the entry
before any HIP call (a HIP call without a device fails with another code and another message), with the outputs untouched; the
R glue registers its two entries, the R wrappers call them, INTEGRATION.md names them, and the host layer exports the new
functions and methods."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_taper_pattern": (r"int\s+cocons_taper_pattern\s*\(\s*int n,\s*const double \*locs,\s*int m,\s*"
                             r"const double \*locs_query[^,]*,\s*double delta,\s*int kind,\s*int device,\s*long long cap,\s*"
                             r"long long \*nnz,\s*int \*rowpointers,\s*int \*colindices,\s*double \*entries\s*\)\s*;", 12),
    "cocons_fit_create_taper_delta": (r"cocons_fit\s*\*\s*cocons_fit_create_taper_delta\s*\(\s*int n,\s*int p,\s*int r,\s*"
                                      r"const double \*locs,\s*const double \*X,\s*const double \*z,\s*"
                                      r"const double \*smooth_limits,\s*int device,\s*double delta,\s*int kind\s*\)\s*;", 10),
    "cocons_krige_taper_apply_delta": (r"int\s+cocons_krige_taper_apply_delta\s*\(\s*cocons_fit\s*\*\s*fit,\s*int m,\s*"
                                       r"const double \*locs_pred,\s*const double \*X_pred,\s*double delta,\s*int kind,\s*"
                                       r"double \*stochastic,\s*double \*quadform,\s*long long \*nnz_out[^)]*\)\s*;", 9),
}


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_headers_declare_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    for name, (pat, nargs) in DECLS.items():
        assert re.search(pat, h), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name)
    for const, value in (("COCONS_TAPER_WEND1", 1), ("COCONS_TAPER_WEND2", 2), ("COCONS_TAPER_SPH", 3)):
        assert re.search(r"#define\s+%s\s+%d\b" % (const, value), h), const
    d = open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read()
    assert re.search(r"int\s+cocons_debug_pattern_cells\s*\(\s*int n,\s*const double \*locs,\s*double delta,\s*int m,\s*"
                     r"const double \*pts,\s*double \*geom5,\s*int \*cells\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_pattern_cells"][1]) == 7 and hasattr(L, "cocons_debug_pattern_cells")
    assert L.cocons_abi_version() == 1


def test_taper_pattern_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    name = "cocons_taper_pattern"
    n, m = 4, 3
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    q = np.array([0.1, 0.2, 0.3, 0.0, 0.0, 0.0])
    bad_locs = locs.copy(); bad_locs[5] = np.nan
    inf_locs = locs.copy(); inf_locs[2] = np.inf
    bad_q = q.copy(); bad_q[4] = -np.inf
    nnz = ctypes.c_longlong(-77)
    rp = np.full(n + 1, -7, dtype=np.int32)
    ci = np.full(64, -7, dtype=np.int32)
    ent = np.full(64, -7.0)

    def call(n_=n, locs_=locs, m_=m, q_=None, delta=1.5, kind=1, nnz_=nnz, rp_=rp, ci_=ci, ent_=ent):
        return L.cocons_taper_pattern(n_, _dp(locs_), m_, _dp(q_), delta, kind, 0, 64,
                                      None if nnz_ is None else ctypes.byref(nnz_), _ip(rp_), _ip(ci_), _dp(ent_))

    cases = (dict(locs_=None), dict(nnz_=None), dict(rp_=None), dict(ent_=None), dict(n_=0), dict(n_=-3),
             dict(q_=q, m_=0), dict(q_=q, m_=-1), dict(delta=0.0), dict(delta=-1.0), dict(delta=np.nan), dict(delta=np.inf),
             dict(kind=0), dict(kind=4), dict(kind=-1), dict(locs_=bad_locs), dict(locs_=inf_locs), dict(q_=bad_q),
             dict(ci_=None, delta=np.nan), dict(ci_=None, kind=7))
    for kw in cases:
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith(name + ":"), (kw, _lib.last_error())
    assert nnz.value == -77 and np.all(rp == -7) and np.all(ci == -7) and np.all(ent == -7.0)


def test_create_and_apply_delta_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    n, p, m = 4, 2, 3
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    bad = locs.copy(); bad[1] = np.nan
    X, z, sl = np.ones(n * p), np.ones(n), np.array([0.5, 2.5])

    def create(n_=n, locs_=locs, X_=X, z_=z, sl_=sl, delta=1.5, kind=2):
        return L.cocons_fit_create_taper_delta(n_, p, 1, _dp(locs_), _dp(X_), _dp(z_), _dp(sl_), 0, delta, kind)

    for kw in (dict(locs_=None), dict(X_=None), dict(z_=None), dict(sl_=None), dict(n_=0), dict(delta=0.0), dict(delta=np.nan),
               dict(delta=-np.inf), dict(kind=0), dict(kind=4), dict(locs_=bad)):
        assert not create(**kw), kw
        assert _lib.last_error().startswith("cocons_fit_create_taper_delta:"), (kw, _lib.last_error())

    name = "cocons_krige_taper_apply_delta"
    lp, Xp = np.zeros(m * 2), np.zeros(m * p)
    bad_lp = lp.copy(); bad_lp[3] = np.inf
    st, qf = np.full(m, 7.0), np.full(m, 7.0)
    nnz = ctypes.c_longlong(-77)

    def apply(m_=m, lp_=lp, Xp_=Xp, delta=0.3, kind=1, st_=st, qf_=qf):
        return L.cocons_krige_taper_apply_delta(None, m_, _dp(lp_), _dp(Xp_), delta, kind, _dp(st_), _dp(qf_), ctypes.byref(nnz))

    assert apply() == -1
    assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
    for kw in (dict(m_=-1), dict(lp_=None), dict(Xp_=None), dict(st_=None), dict(qf_=None), dict(delta=0.0), dict(delta=-2.0),
               dict(delta=np.nan), dict(delta=np.inf), dict(kind=0), dict(kind=4), dict(lp_=bad_lp)):
        assert apply(**kw) == -1, kw
        msg = _lib.last_error()
        assert msg.startswith(name + ":") and "null fit handle" not in msg, (kw, msg)
    assert np.all(st == 7.0) and np.all(qf == 7.0) and nnz.value == -77

    # the diagnostic entry: host only
    geom, cells = np.full(5, -7.0), np.full(2 * m, -7, dtype=np.int32)
    for kw in (dict(n_=0), dict(delta=0.0), dict(delta=np.nan), dict(locs_=bad), dict(locs_=None)):
        a = dict(n_=n, locs_=locs, delta=1.0)
        a.update(kw)
        assert L.cocons_debug_pattern_cells(a["n_"], _dp(a["locs_"]), a["delta"], m, _dp(lp), _dp(geom), _ip(cells)) == -1, kw
        assert _lib.last_error().startswith("cocons_debug_pattern_cells:"), kw
    assert np.all(geom == -7.0) and np.all(cells == -7)


def test_glue_registers_the_entries_and_r_wrappers_call_them():
    from test_glue_exec import RStub
    R = RStub()
    for name, arity in (("_cocons_hip_taper_pattern", 5), ("_cocons_hip_krige_taper_delta", 5)):
        assert R.L.stub_registered_arity(name.encode()) == arity, name
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry in ((r"\.cocons\.hip\.taper\.pattern", "_cocons_hip_taper_pattern"),
                      (r"\.cocons\.hip\.krige\.taper\.delta", "_cocons_hip_krige_taper_delta")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_taper_pattern", "cocons_fit_create_taper_delta", "cocons_krige_taper_apply_delta",
                  "_cocons_hip_taper_pattern", "_cocons_hip_krige_taper_delta", ".cocons.hip.taper.pattern",
                  ".cocons.hip.krige.taper.delta"):
        assert entry in doc, entry


def test_host_layer_exports_the_functions_and_the_methods():
    import cocons_amd as ca
    assert callable(ca.taper_pattern) and callable(ca.cocoPredict_sparse_delta)
    for name in ("from_delta", "krige_taper_core_delta"):
        assert callable(getattr(ca.CoconsTaperFit, name)), name
    import inspect
    sig = inspect.signature(ca.taper_pattern)
    assert list(sig.parameters)[:4] == ["locs", "delta", "kind", "newlocs"] and sig.parameters["kind"].default == "wend1"
    assert "pred_taper" not in inspect.signature(ca.cocoPredict_sparse_delta).parameters
