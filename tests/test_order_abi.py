"""The maxmin ordering at the boundary, without a GPU: the headers declare cocons_vecchia_order, cocons_debug_order_plan and
cocons_debug_order_phases, the library exports them and the ctypes binding carries them; every bad call is refused with -1 and
a message naming the entry before any HIP call (a HIP call without a device fails with another code and another message),
with the outputs untouched; the R glue registers its entry, the R wrapper calls it, INTEGRATION.md names it, and the host layer
exports the new functions and methods."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_headers_declare_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    assert re.search(r"int\s+cocons_vecchia_order\s*\(\s*int n,\s*const double \*locs,\s*int device,\s*int \*order,\s*"
                     r"int \*level_counts[^)]*\)\s*;", h)
    assert len(_lib.SIGNATURES["cocons_vecchia_order"][1]) == 5 and hasattr(L, "cocons_vecchia_order")
    d = open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read()
    assert re.search(r"int\s+cocons_debug_order_plan\s*\(\s*int n,\s*const double \*locs,\s*int \*labels,\s*double \*geom3,\s*"
                     r"double \*levels2\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_order_plan"][1]) == 5 and hasattr(L, "cocons_debug_order_plan")
    assert re.search(r"int\s+cocons_debug_order_phases\s*\(\s*int n,\s*const double \*locs,\s*int device,\s*int binned_from,\s*"
                     r"int \*order,\s*int \*level_counts,\s*double \*ms4,\s*long long \*stats5\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_order_phases"][1]) == 8 and hasattr(L, "cocons_debug_order_phases")
    assert L.cocons_abi_version() == 1
    # the header states the rule: the constants of the labels, the strict conflict, the rest, and the overflow refusal
    for text in ("0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35", "d2 < e_k (strict)", "ldexp(L, 1 - k)", "2^511"):
        assert text in h, text


def test_order_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    name = "cocons_vecchia_order"
    n = 4
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    nan_locs = locs.copy(); nan_locs[5] = np.nan
    inf_locs = locs.copy(); inf_locs[2] = np.inf
    ninf_locs = locs.copy(); ninf_locs[7] = -np.inf
    wide = locs.copy(); wide[0] = -1e160; wide[1] = 1e160          # finite, but the squared span overflows
    order = np.full(n, -7, dtype=np.int32)
    counts = np.full(67, -7, dtype=np.int32)

    def call(n_=n, locs_=locs, order_=order, counts_=counts):
        return L.cocons_vecchia_order(n_, _dp(locs_), 0, _ip(order_), _ip(counts_))

    for kw in (dict(locs_=None), dict(order_=None), dict(n_=0), dict(n_=-3), dict(locs_=nan_locs), dict(locs_=inf_locs),
               dict(locs_=ninf_locs), dict(locs_=wide), dict(locs_=nan_locs, counts_=None)):
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith(name + ":"), (kw, _lib.last_error())
    assert np.all(order == -7) and np.all(counts == -7)
    # the timing entry refuses the same arguments under its own name, and its own, before any HIP call
    ms, st = np.full(4, -7.0), np.full(5, -7, dtype=np.int64)
    sp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    for a in ((0, locs, 0, ms, st), (n, None, 0, ms, st), (n, nan_locs, 0, ms, st), (n, wide, 0, ms, st), (n, locs, -1, ms, st),
              (n, locs, 65, ms, st), (n, locs, 0, None, st), (n, locs, 0, ms, None)):
        assert L.cocons_debug_order_phases(a[0], _dp(a[1]), 0, a[2], _ip(order), _ip(counts), _dp(a[3]), sp(a[4])) == -1, a
        assert _lib.last_error().startswith("cocons_debug_order_phases:"), _lib.last_error()
    assert np.all(order == -7) and np.all(counts == -7) and np.all(ms == -7.0) and np.all(st == -7)
    # and the plan
    lab, geom, lv = np.full(n, -7, dtype=np.int32), np.full(3, -7.0), np.full(128, -7.0)
    for a in ((0, locs, lab, geom, lv), (n, None, lab, geom, lv), (n, locs, None, geom, lv), (n, locs, lab, None, lv),
              (n, locs, lab, geom, None), (n, nan_locs, lab, geom, lv), (n, wide, lab, geom, lv)):
        assert L.cocons_debug_order_plan(a[0], _dp(a[1]), _ip(a[2]), _dp(a[3]), _dp(a[4])) == -1, a
        assert _lib.last_error().startswith("cocons_debug_order_plan:"), _lib.last_error()
    assert np.all(lab == -7) and np.all(geom == -7.0) and np.all(lv == -7.0)


def test_python_layer_refuses_and_exports():
    import cocons_amd as ca
    from cocons_amd import _lib
    for name in ("vecchia_order", "vecchia_order_device"):
        assert callable(getattr(ca, name)), name
    assert list(inspect.signature(ca.vecchia_order).parameters)[0] == "locs"
    sig = inspect.signature(ca.vecchia_order_device)
    assert list(sig.parameters) == ["locs", "device", "levels"]
    assert sig.parameters["device"].default == 0 and sig.parameters["levels"].default is False
    sig = inspect.signature(ca.CoconsVecchiaFit.from_maxmin)
    assert list(sig.parameters) == ["locs", "x_covariates", "z", "smooth_limits", "m", "device"]
    for name in ("to_maxmin", "from_maxmin_order"):
        assert callable(getattr(ca.CoconsVecchiaFit, name)), name
    assert not hasattr(ca.CoconsFit, "maxmin_order")          # the permutation's name collides with nothing on the dense handle
    with pytest.raises(_lib.CoconsHipError, match="cocons_vecchia_order: a coordinate of locs is not finite"):
        ca.vecchia_order_device(np.array([[0.0, 1.0], [np.nan, 2.0]]))
    # the existing functions keep their signatures
    assert list(inspect.signature(ca.vecchia_neighbours_device).parameters)[:2] == ["locs", "m"]
    assert list(inspect.signature(ca.CoconsVecchiaFit.from_knn).parameters) == ["locs", "x_covariates", "z", "smooth_limits",
                                                                               "m", "device"]


def test_glue_registers_the_entry_and_the_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_vecchia_order") == 2
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.vecchia\.order <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_vecchia_order`" in m.group(2)
    assert [a.split("=")[0].strip() for a in m.group(1).split(",")] == ["locs", "device"]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_vecchia_order", "_cocons_hip_vecchia_order", ".cocons.hip.vecchia.order", "from_maxmin"):
        assert entry in doc, entry
    walk = doc[doc.index("**The Vecchia approximation**"):doc.index("**The neighbour search on the device**")]
    assert "ord <- .cocons.hip.vecchia.order(locs)" in walk and "GpGp::order_maxmin" not in walk
    bad = np.array([[0.0, 1.0], [np.inf, 2.0], [3.0, 4.0]])
    with pytest.raises(RuntimeError, match="cocons_vecchia_order: a coordinate of locs is not finite"):
        R.call("_cocons_hip_vecchia_order", R.real(bad), R.integer([0]))
    with pytest.raises(RuntimeError, match="locs must be a double matrix with 2 columns"):
        R.call("_cocons_hip_vecchia_order", R.real(bad[:, 0]), R.integer([0]))
