"""U^-T on a Vecchia fit at the boundary, without a GPU: the header declares cocons_vecchia_unwhiten_t,
cocons_vecchia_cov_mult, cocons_vecchia_cov_cols and cocons_vecchia_schedule_t, the library exports them (nm -D) and the ctypes
binding carries them; every call that can be refused on its arguments alone is refused with -1 and a message that starts with
the entry's name, before any HIP call (a HIP call without a device fails with another code and another message), with the
outputs untouched; the diagnostics header gives the tiers' constants; the R glue registers its four shims with their arities,
the R wrappers exist with their argument lists, the documents name the entries, and the host layer exports the new function and
methods.  (The refusals that need a handle's n -- n_fixed >= n, an index beyond n, another kind of handle, grouped = 1 without
a plan -- are in tests/test_gpu_vecchia_cov.py.)"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_vecchia_unwhiten_t": (r"int\s+cocons_vecchia_unwhiten_t\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int grouped,\s*"
                                  r"int c,\s*const double \*W\s*(?:/\*.*?\*/)?\s*,\s*double \*out\s*(?:/\*.*?\*/)?\s*\)\s*;", 6),
    "cocons_vecchia_cov_mult": (r"int\s+cocons_vecchia_cov_mult\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int grouped,\s*"
                                r"int n_fixed,\s*int c,\s*const double \*B\s*(?:/\*.*?\*/)?\s*,\s*double \*out\s*(?:/\*.*?\*/)?\s*\)\s*;", 7),
    "cocons_vecchia_cov_cols": (r"int\s+cocons_vecchia_cov_cols\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int grouped,\s*"
                                r"int n_fixed,\s*int nidx,\s*const int \*idx\s*(?:/\*.*?\*/)?\s*,\s*double \*out\s*(?:/\*.*?\*/)?\s*\)\s*;", 7),
    "cocons_vecchia_schedule_t": (r"int\s+cocons_vecchia_schedule_t\s*\(\s*cocons_fit\s*\*\s*fit,\s*int n_fixed,\s*int \*tlevels\s*"
                                  r"(?:/\*.*?\*/)?\s*,\s*long long \*out4\s*\)\s*;", 4),
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
        assert re.search(pat, h), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name)
        assert re.search(r" T %s$" % name, exported, re.M), name
    d = open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read()
    assert re.search(r"int\s+cocons_debug_vecchia_solve_t_tiers\s*\(\s*int \*out4\s*\)\s*;", d)
    assert L.cocons_abi_version() == 1


def test_the_tiers_are_read_through_the_diagnostics_header():
    from cocons_amd import _lib
    L = _lib.load()
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    assert L.cocons_debug_vecchia_solve_t_tiers(None) == -1
    assert _lib.last_error().startswith("cocons_debug_vecchia_solve_t_tiers:")
    assert L.cocons_debug_vecchia_solve_t_tiers(out) == 0
    wide, threads, cols, items = list(out)
    k = open(os.path.join(ROOT, "cocons_amd", "csrc", "kernels.h")).read()
    for name, v in (("VECCHIA_SOLVE_T_WIDE", wide), ("VECCHIA_SOLVE_T_WIDE_THREADS", threads), ("VECCHIA_SOLVE_T_COLS", cols),
                    ("VECCHIA_SOLVE_T_FUSE_ITEMS", items)):
        assert re.search(r"constexpr int %s = %d;" % (name, v), k), name
    # a list past the threshold gives every thread of the workgroup at least one entry; a wavefront's worth at the least
    assert wide >= threads >= 64 and threads % 64 == 0 and cols >= 1 and items >= 1


def test_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p, n, c = 2, 5, 2
    theta = np.zeros(6 * p)
    W, out = np.ones(n * c), np.full(n * c, 7.0)
    idx = np.array([1, 5], dtype=np.int32)
    fake = ctypes.c_void_p(1)           # never dereferenced: every case below is refused on its arguments alone

    def unwhiten_t(f=fake, theta_=theta, grouped=0, c_=c, W_=W, out_=out):
        return L.cocons_vecchia_unwhiten_t(f, _dp(theta_), grouped, c_, _dp(W_), _dp(out_))

    def cov_mult(f=fake, theta_=theta, grouped=0, n_fixed=0, c_=c, W_=W, out_=out):
        return L.cocons_vecchia_cov_mult(f, _dp(theta_), grouped, n_fixed, c_, _dp(W_), _dp(out_))

    def cov_cols(f=fake, theta_=theta, grouped=0, n_fixed=0, nidx=2, idx_=idx, out_=out):
        return L.cocons_vecchia_cov_cols(f, _dp(theta_), grouped, n_fixed, nidx, _ip(idx_), _dp(out_))

    levels, out4 = np.full(n, -7, dtype=np.int32), (ctypes.c_longlong * 4)(-7, -7, -7, -7)

    def schedule_t(f=fake, n_fixed=0, out4_=out4):
        return L.cocons_vecchia_schedule_t(f, n_fixed, _ip(levels), out4_)

    for fn, name, cases in (
            (unwhiten_t, "cocons_vecchia_unwhiten_t", (dict(theta_=None), dict(W_=None), dict(out_=None), dict(c_=0), dict(c_=-2),
                                                       dict(grouped=2), dict(grouped=-1))),
            (cov_mult, "cocons_vecchia_cov_mult", (dict(theta_=None), dict(W_=None), dict(out_=None), dict(c_=0), dict(c_=-2),
                                                   dict(grouped=2), dict(grouped=-1), dict(n_fixed=-1))),
            (cov_cols, "cocons_vecchia_cov_cols", (dict(theta_=None), dict(idx_=None), dict(out_=None), dict(nidx=0), dict(nidx=-1),
                                                   dict(grouped=2), dict(grouped=-1), dict(n_fixed=-1),
                                                   dict(idx_=np.array([0, 3], dtype=np.int32)),
                                                   dict(idx_=np.array([3, -2], dtype=np.int32)),
                                                   dict(n_fixed=3, idx_=np.array([4, 3], dtype=np.int32)))),
            (schedule_t, "cocons_vecchia_schedule_t", (dict(out4_=None), dict(n_fixed=-1)))):
        assert fn(f=None) == -1
        assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
        for kw in cases:
            assert fn(**kw) == -1, (name, kw)
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and "null fit handle" not in msg, (name, kw, msg)
    assert np.all(out == 7.0) and np.all(levels == -7) and list(out4) == [-7] * 4
    assert "c = 0" in (unwhiten_t(c_=0), _lib.last_error())[1]
    assert "grouped = 2" in (cov_mult(grouped=2), _lib.last_error())[1]
    assert "n_fixed = -1" in (cov_mult(n_fixed=-1), _lib.last_error())[1]
    assert "nidx = 0" in (cov_cols(nidx=0), _lib.last_error())[1]
    assert "idx[1] = 3" in (cov_cols(n_fixed=3, idx_=np.array([4, 3], dtype=np.int32)), _lib.last_error())[1]


def test_glue_registers_the_shims_and_r_wrappers_exist():
    from test_glue_exec import RStub
    R = RStub()
    for name, arity in (("_cocons_hip_vecchia_unwhiten_t", 4), ("_cocons_hip_vecchia_cov_mult", 5),
                        ("_cocons_hip_vecchia_cov_cols", 5), ("_cocons_hip_vecchia_schedule_t", 2)):
        assert R.L.stub_registered_arity(name.encode()) == arity, name
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry, args in ((r"\.cocons\.hip\.vecchia\.unwhiten\.t", "_cocons_hip_vecchia_unwhiten_t", "fit, theta_list, W, grouped = FALSE"),
                            (r"\.cocons\.hip\.vecchia\.cov\.mult", "_cocons_hip_vecchia_cov_mult",
                             "fit, theta_list, B, n_fixed = 0L, grouped = FALSE"),
                            (r"\.cocons\.hip\.vecchia\.cov\.cols", "_cocons_hip_vecchia_cov_cols",
                             "fit, theta_list, idx, n_fixed = 0L, grouped = FALSE"),
                            (r"\.cocons\.hip\.vecchia\.schedule\.t", "_cocons_hip_vecchia_schedule_t", "fit, n_fixed = 0L")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
        assert m.group(1) == args, (fn, m.group(1))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_vecchia_unwhiten_t", "cocons_vecchia_cov_mult", "cocons_vecchia_cov_cols", "cocons_vecchia_schedule_t",
                  "_cocons_hip_vecchia_unwhiten_t", "_cocons_hip_vecchia_cov_mult", "_cocons_hip_vecchia_cov_cols",
                  "_cocons_hip_vecchia_schedule_t", ".cocons.hip.vecchia.unwhiten.t", ".cocons.hip.vecchia.cov.mult",
                  ".cocons.hip.vecchia.cov.cols", ".cocons.hip.vecchia.schedule.t"):
        assert entry in doc, entry
    assert "4ad" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "cocons_vecchia_cov_mult" in open(os.path.join(ROOT, "README.md")).read()


def test_host_layer_exports_the_function_and_the_methods():
    import cocons_amd as ca
    assert callable(ca.cocoPredict_vecchia_joint)
    sig = inspect.signature(ca.cocoPredict_vecchia_joint)
    assert list(sig.parameters) == ["theta_list", "locs", "newlocs", "X_std", "X_pred_std", "smooth_limits", "z", "m", "cov_idx", "fit"]
    assert sig.parameters["cov_idx"].default is None and sig.parameters["fit"].default is None
    for name, params, defaults in (("unwhiten_t_core", ["theta_list", "W", "grouped"], {"grouped": False}),
                                   ("cov_mult_core", ["theta_list", "B", "n_fixed", "grouped"], {"n_fixed": 0, "grouped": False}),
                                   ("cov_cols_core", ["theta_list", "idx", "n_fixed", "grouped"], {"n_fixed": 0, "grouped": False}),
                                   ("schedule_t", ["n_fixed"], {"n_fixed": 0})):
        sig = inspect.signature(getattr(ca.CoconsVecchiaFit, name))
        assert list(sig.parameters)[1:] == params, name
        for k, v in defaults.items():
            assert sig.parameters[k].default == v, (name, k)
    # the existing methods keep their signatures
    assert list(inspect.signature(ca.CoconsVecchiaFit.whiten_t_core).parameters)[1:] == ["theta_list", "W"]
    assert list(inspect.signature(ca.CoconsVecchiaFit.unwhiten_core).parameters)[1:] == ["theta_list", "W"]
