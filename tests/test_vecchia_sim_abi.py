"""U^-1 on a Vecchia fit at the boundary, without a GPU: the header declares cocons_vecchia_unwhiten, cocons_sim_vecchia and
cocons_vecchia_schedule, the library exports them (nm -D) and the ctypes binding carries them; every call that can be refused
on its arguments alone is refused with -1 and a message that starts with the entry's name, before any HIP call (a HIP call
without a device fails with another code and another message), with the outputs untouched; the R glue registers its three
shims with their arities, the R wrappers exist with their argument lists, the documents name the entries, and the host layer
exports the new functions and methods.  (The refusals that need a handle's n and r -- n_fixed >= n, z_col >= r, another kind
of handle -- are in tests/test_gpu_vecchia_sim.py.)"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "cocons_vecchia_unwhiten": (r"int\s+cocons_vecchia_unwhiten\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int c,\s*"
                                r"const double \*W,\s*double \*out\s*\)\s*;", 5),
    "cocons_sim_vecchia": (r"int\s+cocons_sim_vecchia\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*"
                           r"int n_fixed,\s*int z_col,\s*int nsim,\s*const double \*iiderrors,\s*double \*out\s*\)\s*;", 8),
    "cocons_vecchia_schedule": (r"int\s+cocons_vecchia_schedule\s*\(\s*cocons_fit\s*\*\s*fit,\s*int n_fixed,\s*int \*levels\s*(?:/\*.*?\*/)?\s*,\s*"
                                r"long long \*out4\s*\)\s*;", 4),
}


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


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
    assert re.search(r"int\s+cocons_debug_vecchia_sim_phases\s*\(\s*struct cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int c,\s*"
                     r"const double \*W,\s*double \*out,\s*double \*ms3\s*\)\s*;", d)
    assert len(_lib.DIAG_SIGNATURES["cocons_debug_vecchia_sim_phases"][1]) == 6 and hasattr(L, "cocons_debug_vecchia_sim_phases")
    assert L.cocons_abi_version() == 1


def test_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p, n, c = 2, 5, 2
    theta, mean = np.zeros(6 * p), np.zeros(p)
    W, out = np.ones(n * c), np.full(n * c, 7.0)
    fake = ctypes.c_void_p(1)           # never dereferenced: every case below is refused on its arguments alone

    def unwhiten(f=fake, theta_=theta, c_=c, W_=W, out_=out):
        return L.cocons_vecchia_unwhiten(f, _dp(theta_), c_, _dp(W_), _dp(out_))

    def sim(f=fake, theta_=theta, mean_=mean, n_fixed=0, z_col=0, nsim=c, E=W, out_=out):
        return L.cocons_sim_vecchia(f, _dp(theta_), _dp(mean_), n_fixed, z_col, nsim, _dp(E), _dp(out_))

    levels, out4 = np.full(n, -7, dtype=np.int32), (ctypes.c_longlong * 4)(-7, -7, -7, -7)

    def schedule(f=fake, n_fixed=0, out4_=out4):
        return L.cocons_vecchia_schedule(f, n_fixed, levels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), out4_)

    for fn, name, cases in (
            (unwhiten, "cocons_vecchia_unwhiten", (dict(theta_=None), dict(W_=None), dict(out_=None), dict(c_=0), dict(c_=-2))),
            (sim, "cocons_sim_vecchia", (dict(theta_=None), dict(mean_=None), dict(E=None), dict(out_=None), dict(nsim=0),
                                         dict(nsim=-1), dict(n_fixed=-1), dict(z_col=-1))),
            (schedule, "cocons_vecchia_schedule", (dict(out4_=None), dict(n_fixed=-1)))):
        assert fn(f=None) == -1
        assert _lib.last_error().startswith(name + ":") and "null fit handle" in _lib.last_error()
        for kw in cases:
            assert fn(**kw) == -1, (name, kw)
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and "null fit handle" not in msg, (name, kw, msg)
    assert np.all(out == 7.0) and np.all(levels == -7) and list(out4) == [-7] * 4
    assert "c = 0" in (unwhiten(c_=0), _lib.last_error())[1]
    assert "nsim = 0" in (sim(nsim=0), _lib.last_error())[1]
    assert "n_fixed = -1" in (sim(n_fixed=-1), _lib.last_error())[1]
    assert "z_col = -1" in (sim(z_col=-1), _lib.last_error())[1]
    # the timing entry of the diagnostics refuses the same arguments under its own name
    ms = np.full(3, -7.0)
    for a in ((None, theta, c, W, out, ms), (fake, None, c, W, out, ms), (fake, theta, 0, W, out, ms), (fake, theta, c, None, out, ms),
              (fake, theta, c, W, None, ms), (fake, theta, c, W, out, None)):
        assert L.cocons_debug_vecchia_sim_phases(a[0], _dp(a[1]), a[2], _dp(a[3]), _dp(a[4]), _dp(a[5])) == -1, a
        assert _lib.last_error().startswith("cocons_debug_vecchia_sim_phases:"), _lib.last_error()
    assert np.all(ms == -7.0) and np.all(out == 7.0)


def test_glue_registers_the_shims_and_r_wrappers_exist():
    from test_glue_exec import RStub
    R = RStub()
    for name, arity in (("_cocons_hip_vecchia_unwhiten", 3), ("_cocons_hip_vecchia_sim", 5), ("_cocons_hip_vecchia_schedule", 2)):
        assert R.L.stub_registered_arity(name.encode()) == arity, name
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for fn, entry, args in ((r"\.cocons\.hip\.vecchia\.unwhiten", "_cocons_hip_vecchia_unwhiten", "fit, theta_list, W"),
                            (r"\.cocons\.hip\.vecchia\.sim", "_cocons_hip_vecchia_sim",
                             "fit, theta_list, iiderrors, n_fixed = 0L, z_col = 1L"),
                            (r"\.cocons\.hip\.vecchia\.schedule", "_cocons_hip_vecchia_schedule", "fit, n_fixed = 0L")):
        m = re.search(fn + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert m and ("`%s`" % entry) in m.group(2), fn
        assert m.group(1) == args, (fn, m.group(1))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_vecchia_unwhiten", "cocons_sim_vecchia", "cocons_vecchia_schedule", "_cocons_hip_vecchia_unwhiten",
                  "_cocons_hip_vecchia_sim", "_cocons_hip_vecchia_schedule", ".cocons.hip.vecchia.unwhiten",
                  ".cocons.hip.vecchia.sim", ".cocons.hip.vecchia.schedule"):
        assert entry in doc, entry
    assert "4v" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_host_layer_exports_the_functions_and_the_methods():
    import cocons_amd as ca
    for name in ("cocoSim_vecchia", "cocoSim_cond_vecchia"):
        assert callable(getattr(ca, name)), name
    for name in ("unwhiten_core", "sim_core", "schedule"):
        assert callable(getattr(ca.CoconsVecchiaFit, name)), name
    assert list(inspect.signature(ca.CoconsVecchiaFit.unwhiten_core).parameters)[1:] == ["theta_list", "W"]
    sig = inspect.signature(ca.CoconsVecchiaFit.sim_core)
    assert list(sig.parameters)[1:] == ["theta_list", "iiderrors", "n_fixed", "z_col"]
    assert sig.parameters["n_fixed"].default == 0 and sig.parameters["z_col"].default == 0
    sig = inspect.signature(ca.CoconsVecchiaFit.schedule)
    assert list(sig.parameters)[1:] == ["n_fixed"] and sig.parameters["n_fixed"].default == 0
    sig = inspect.signature(ca.cocoSim_vecchia)
    assert list(sig.parameters) == ["theta_list", "locs", "X_std", "smooth_limits", "iiderrors", "nn", "m", "fit"]
    assert all(sig.parameters[k].default is None for k in ("nn", "m", "fit"))
    sig = inspect.signature(ca.cocoSim_cond_vecchia)
    assert list(sig.parameters) == ["theta_list", "locs", "newlocs", "X_std", "X_pred_std", "smooth_limits", "z", "iiderrors", "m",
                                    "fit"]
    # the existing methods keep their signatures
    assert list(inspect.signature(ca.CoconsVecchiaFit.whiten_core).parameters)[1:] == ["theta_list", "B"]
