"""U' and cross-validation on a Vecchia fit at the boundary, without a GPU: the header declares cocons_vecchia_transpose,
cocons_vecchia_whiten_t and cocons_cv_vecchia, the library exports them (nm -D) and the ctypes binding carries them; every
call that can be refused on its arguments alone is refused with -1 and a message that starts with the entry's name, before
any HIP call, with the outputs untouched; the R glue registers its three shims with their arities, the R wrappers exist with
their argument lists, the documents name the entries, and the host layer exports the new function and methods.  (The
refusals that need a handle's n -- labels, fold sizes, another kind of handle -- are in tests/test_gpu_vecchia_cv.py.)"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = r"\s*(?:/\*.*?\*/)?\s*"

DECLS = {
    "cocons_vecchia_transpose": (r"int\s+cocons_vecchia_transpose\s*\(\s*cocons_fit\s*\*\s*fit,\s*int \*ptr" + C + r",\s*int \*rows" + C +
                                 r",\s*long long \*out4\s*\)\s*;", 4),
    "cocons_vecchia_whiten_t": (r"int\s+cocons_vecchia_whiten_t\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int c,\s*"
                                r"const double \*W,\s*double \*out" + C + r",\s*double \*qdiag" + C + r"\)\s*;", 6),
    "cocons_cv_vecchia": (r"int\s+cocons_cv_vecchia\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
                          r"int nfold,\s*const int \*fold,\s*double \*resid" + C + r",\s*double \*var" + C +
                          r",\s*long long \*stats4" + C + r"\)\s*;", 8),
}


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name, (pat, nargs) in DECLS.items():
        assert re.search(pat, h, re.S), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name)
        assert re.search(r" T %s$" % name, exported, re.M), name
    d = open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read()
    assert re.search(r"int\s+cocons_debug_vecchia_transpose_phases\s*\(\s*struct cocons_fit\s*\*\s*fit,\s*double \*ms4\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_vecchia_transpose_phases"][1]) == 2
    assert hasattr(L, "cocons_debug_vecchia_transpose_phases")
    assert L.cocons_abi_version() == 1
    # the header states the definitions every reference follows, and that U b need not be the whitening entry's bits
    for text in ("Transposed lists", "Fold block", "own row first|own row's term", "need not be cocons_vecchia_whiten's bits",
                 "No floating-point atomics", "a fold of one returns leave-one-out's bits"):
        assert re.search(text, h), text


def test_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p, n, c = 2, 5, 2
    theta, mean = np.zeros(6 * p), np.zeros(p)
    W, out, qd = np.ones(n * c), np.full(n * c, 7.0), np.full(n, 7.0)
    resid, var = np.full(n * c, 7.0), np.full(n, 7.0)
    fold = np.zeros(n, dtype=np.int32)
    ptr, rows = np.full(n + 1, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32)
    out4, st4 = (ctypes.c_longlong * 4)(-7, -7, -7, -7), (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    fake = ctypes.c_void_p(1)           # never dereferenced: every case below is refused on its arguments alone

    def transpose(f=fake, out4_=out4):
        return L.cocons_vecchia_transpose(f, _ip(ptr), _ip(rows), out4_)

    def whiten_t(f=fake, theta_=theta, c_=c, W_=W, out_=out):
        return L.cocons_vecchia_whiten_t(f, _dp(theta_), c_, _dp(W_), _dp(out_), _dp(qd))

    def cv(f=fake, theta_=theta, mean_=mean, nfold=0, fold_=None, resid_=resid, var_=var):
        return L.cocons_cv_vecchia(f, _dp(theta_), _dp(mean_), nfold, _ip(fold_), _dp(resid_), _dp(var_), st4)

    for fn, name, cases in (
            (transpose, "cocons_vecchia_transpose", (dict(out4_=None),)),
            (whiten_t, "cocons_vecchia_whiten_t", (dict(theta_=None), dict(W_=None), dict(out_=None), dict(c_=0), dict(c_=-2))),
            (cv, "cocons_cv_vecchia", (dict(theta_=None), dict(mean_=None), dict(resid_=None), dict(var_=None), dict(nfold=-1),
                                       dict(nfold=3), dict(nfold=0, fold_=fold)))):
        assert fn(f=None) == -1
        assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
        for kw in cases:
            assert fn(**kw) == -1, (name, kw)
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and "null fit handle" not in msg, (name, kw, msg)
    for a in (out, qd, resid, var):
        assert np.all(a == 7.0)
    assert np.all(ptr == -7) and np.all(rows == -7) and list(out4) == [-7] * 4 and list(st4) == [-7] * 4
    assert "c = 0" in (whiten_t(c_=0), _lib.last_error())[1]
    assert "nfold = -1" in (cv(nfold=-1), _lib.last_error())[1]
    assert "fold and nfold disagree" in (cv(nfold=3), _lib.last_error())[1]
    ms = np.full(4, -7.0)
    assert L.cocons_debug_vecchia_transpose_phases(None, _dp(ms)) == -1
    assert L.cocons_debug_vecchia_transpose_phases(fake, None) == -1
    assert _lib.last_error().startswith("cocons_debug_vecchia_transpose_phases:") and np.all(ms == -7.0)


def test_glue_registers_the_shims_and_r_wrappers_exist():
    from test_glue_exec import RStub
    R = RStub()
    for name, arity in (("_cocons_hip_vecchia_transpose", 1), ("_cocons_hip_vecchia_whiten_t", 3), ("_cocons_hip_vecchia_cv", 3)):
        assert R.L.stub_registered_arity(name.encode()) == arity, name
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry, args in ((r"\.cocons\.hip\.vecchia\.transpose", "_cocons_hip_vecchia_transpose", "fit"),
                            (r"\.cocons\.hip\.vecchia\.whiten\.t", "_cocons_hip_vecchia_whiten_t", "fit, theta_list, W"),
                            (r"\.cocons\.hip\.vecchia\.cv", "_cocons_hip_vecchia_cv", "fit, theta_list, fold = NULL, safe = TRUE")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
        assert m.group(1) == args, (fn, m.group(1))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_vecchia_transpose", "cocons_vecchia_whiten_t", "cocons_cv_vecchia", "_cocons_hip_vecchia_transpose",
                  "_cocons_hip_vecchia_whiten_t", "_cocons_hip_vecchia_cv", ".cocons.hip.vecchia.transpose",
                  ".cocons.hip.vecchia.whiten.t", ".cocons.hip.vecchia.cv", "cocoCV_vecchia"):
        assert entry in doc, entry
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^### 4x\. ", design, re.M) and "cocons_cv_vecchia" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "cocoCV_vecchia" in readme and "tools/vecchia_cv_timing.py" in readme


def test_host_layer_exports_the_function_and_the_methods():
    import cocons_amd as ca
    assert callable(ca.cocoCV_vecchia)
    for name in ("transpose", "whiten_t_core", "cv_core"):
        assert callable(getattr(ca.CoconsVecchiaFit, name)), name
    assert list(inspect.signature(ca.CoconsVecchiaFit.transpose).parameters) == ["self"]
    assert list(inspect.signature(ca.CoconsVecchiaFit.whiten_t_core).parameters)[1:] == ["theta_list", "W"]
    sig = inspect.signature(ca.CoconsVecchiaFit.cv_core)
    assert list(sig.parameters)[1:3] == ["theta_list", "fold"] and sig.parameters["fold"].default is None
    sig = inspect.signature(ca.cocoCV_vecchia)
    assert list(sig.parameters) == ["theta_list", "locs", "X_std", "smooth_limits", "z", "nn", "m", "fold", "fit"]
    assert all(sig.parameters[k].default is None for k in ("nn", "m", "fold", "fit"))
    # the existing methods keep their signatures
    assert list(inspect.signature(ca.CoconsVecchiaFit.whiten_core).parameters)[1:] == ["theta_list", "B"]
    assert list(inspect.signature(ca.CoconsVecchiaFit.unwhiten_core).parameters)[1:] == ["theta_list", "W"]
