"""The grouped U^-1, U' and cross-validation entries at the boundary, without a GPU, in the pattern of
tests/test_vecchia_group_fisher_abi.py: the header declares each entry with its twin's argument list and the sentence "returns
the bits of <twin> on the same handle", the library exports them (nm -D) and the ctypes bindings carry the twins' signatures;
every call that can be refused on its arguments alone is refused with -1 and the twin's message under the entry's own name,
with the outputs untouched; the R glue registers the shims with the twins' arities and the R wrappers route through the
twins' code; the documents name the entries and the tool; and the host layer has the new methods and functions while the pinned
signatures stand.  (The refusals that need a handle are in tests/test_gpu_vecchia_group_coef.py.)"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = r"\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*"
C = r"(?:/\*.*?\*/)?\s*"            # a comment behind an argument
ARGS = {
    "cocons_vecchia_unwhiten": FIT + r"int c,\s*const double \*W,\s*double \*out\s*\)\s*;",
    "cocons_sim_vecchia": FIT + r"const double \*mean,\s*int n_fixed,\s*int z_col,\s*int nsim,\s*const double \*iiderrors,\s*"
                                r"double \*out\s*\)\s*;",
    "cocons_vecchia_whiten_t": FIT + r"int c,\s*const double \*W,\s*double \*out\s*" + C + r",\s*double \*qdiag\s*" + C + r"\)\s*;",
    "cocons_cv_vecchia": FIT + r"const double \*mean,\s*int nfold,\s*const int \*fold,\s*double \*resid\s*" + C +
                         r",\s*double \*var\s*" + C + r",\s*long long \*stats4\s*" + C + r"\)\s*;",
}
TWINS = tuple(ARGS)
DEBUG, DEBUG_TWIN = "cocons_debug_vecchia_sim_phases_grouped", "cocons_debug_vecchia_sim_phases"


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


@pytest.mark.parametrize("twin", TWINS)
def test_header_declares_binding_has_library_exports(twin):
    from cocons_amd import _lib
    entry = twin + "_grouped"
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"int\s+" + entry + ARGS[twin], h, re.S), entry
    assert re.search(r"int\s+" + twin + ARGS[twin], h, re.S), twin                      # the same argument list
    assert _lib.SIGNATURES[entry] == _lib.SIGNATURES[twin]
    assert hasattr(L, entry)
    assert re.search(r" T %s$" % entry, exported, re.M)
    assert re.search(entry + r"\s+returns\s+the\s+bits\s+of\s*\*?\s*" + twin + r"\s+on\s+the\s+same\s+handle", h), entry
    assert re.search(r"a handle without\s*\*?\s*a plan", h)
    assert L.cocons_abi_version() == 1


def test_the_debug_twin_is_declared_bound_and_exported():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip_diag.h")).read()
    args = (r"\s*\(\s*struct cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int c,\s*const double \*W,\s*double \*out,\s*"
            r"double \*ms3\s*\)\s*;")
    assert re.search(r"int\s+" + DEBUG + args, h, re.S) and re.search(r"int\s+" + DEBUG_TWIN + args, h, re.S)
    assert _lib.DIAG_SIGNATURES[DEBUG] == _lib.DIAG_SIGNATURES[DEBUG_TWIN]
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T %s$" % DEBUG, exported, re.M)


def test_refusals_without_the_gpu():
    """every refusal the twins make before they look at the handle, with the twin's message under the entry's own name"""
    from cocons_amd import _lib
    L = _lib.load()
    n, p = 5, 3
    theta, mean = np.zeros(6 * p), np.zeros(p)
    W, out, qd = np.ones((n, 2), order="F"), np.full((n, 2), 7.0, order="F"), np.full(n, 7.0)
    var, ms3 = np.full(n, 7.0), np.full(3, 7.0)
    fold = np.zeros(n, dtype=np.int32)
    ip = fold.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    fake = ctypes.c_void_p(1)           # never dereferenced: every case below is refused on its arguments alone

    def both(name, call, message):
        """`call(entry function)` on the twin and on the grouped entry: -1 and the same message under either name"""
        for entry in (name, name + "_grouped"):
            assert call(getattr(L, entry)) == -1, (entry, message)
            assert _lib.last_error() == entry + ": " + message, (entry, _lib.last_error())

    # cocons_vecchia_unwhiten and the timed form
    both("cocons_vecchia_unwhiten", lambda f: f(None, _dp(theta), 2, _dp(W), _dp(out)), "null fit handle")
    for a in ((None, 2, _dp(W), _dp(out)), (_dp(theta), 2, None, _dp(out)), (_dp(theta), 2, _dp(W), None)):
        both("cocons_vecchia_unwhiten", lambda f: f(fake, *a), "null argument")
    for c in (0, -3):
        both("cocons_vecchia_unwhiten", lambda f: f(fake, _dp(theta), c, _dp(W), _dp(out)),
             "c = %d (at least one column expected)" % c)
    for entry in (DEBUG_TWIN, DEBUG):
        f = getattr(L, entry)
        assert f(None, _dp(theta), 2, _dp(W), _dp(out), _dp(ms3)) == -1 and _lib.last_error() == entry + ": null fit handle"
        assert f(fake, _dp(theta), 2, _dp(W), _dp(out), None) == -1 and _lib.last_error() == entry + ": null argument"
        assert f(fake, _dp(theta), 0, _dp(W), _dp(out), _dp(ms3)) == -1
        assert _lib.last_error() == entry + ": c = 0 (at least one column expected)"
    # cocons_sim_vecchia
    sim = "cocons_sim_vecchia"
    both(sim, lambda f: f(None, _dp(theta), _dp(mean), 0, 0, 2, _dp(W), _dp(out)), "null fit handle")
    for a in ((None, _dp(mean), 0, 0, 2, _dp(W), _dp(out)), (_dp(theta), None, 0, 0, 2, _dp(W), _dp(out)),
              (_dp(theta), _dp(mean), 0, 0, 2, None, _dp(out)), (_dp(theta), _dp(mean), 0, 0, 2, _dp(W), None)):
        both(sim, lambda f: f(fake, *a), "null argument")
    both(sim, lambda f: f(fake, _dp(theta), _dp(mean), 0, 0, 0, _dp(W), _dp(out)), "nsim = 0 (at least one field expected)")
    both(sim, lambda f: f(fake, _dp(theta), _dp(mean), -1, 0, 2, _dp(W), _dp(out)), "n_fixed = -1 is outside 0 .. n - 1")
    both(sim, lambda f: f(fake, _dp(theta), _dp(mean), 0, -2, 2, _dp(W), _dp(out)), "z_col = -2 is outside the realisations")
    # cocons_vecchia_whiten_t
    wt = "cocons_vecchia_whiten_t"
    both(wt, lambda f: f(None, _dp(theta), 2, _dp(W), _dp(out), _dp(qd)), "null fit handle")
    for a in ((None, 2, _dp(W), _dp(out), _dp(qd)), (_dp(theta), 2, None, _dp(out), _dp(qd)), (_dp(theta), 2, _dp(W), None, _dp(qd))):
        both(wt, lambda f: f(fake, *a), "null argument")
    both(wt, lambda f: f(fake, _dp(theta), 0, _dp(W), _dp(out), _dp(qd)), "c = 0 (at least one column expected)")
    # cocons_cv_vecchia
    cv = "cocons_cv_vecchia"
    both(cv, lambda f: f(None, _dp(theta), _dp(mean), 0, None, _dp(out), _dp(var), None), "null fit handle")
    for a in ((None, _dp(mean), 0, None, _dp(out), _dp(var), None), (_dp(theta), None, 0, None, _dp(out), _dp(var), None),
              (_dp(theta), _dp(mean), 0, None, None, _dp(var), None), (_dp(theta), _dp(mean), 0, None, _dp(out), None, None)):
        both(cv, lambda f: f(fake, *a), "null argument")
    both(cv, lambda f: f(fake, _dp(theta), _dp(mean), -1, ip, _dp(out), _dp(var), None), "nfold = -1 is negative")
    for nfold, lab in ((2, None), (0, ip)):
        both(cv, lambda f: f(fake, _dp(theta), _dp(mean), nfold, lab, _dp(out), _dp(var), None),
             "fold and nfold disagree (fold = NULL with nfold = 0 is leave-one-out)")
    assert np.all(out == 7.0) and np.all(qd == 7.0) and np.all(var == 7.0) and np.all(ms3 == 7.0)


def test_glue_registers_the_shims_and_the_r_wrappers_route_through_the_twins():
    from test_glue_exec import RStub
    R = RStub()
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    glue = open(os.path.join(ROOT, "glue", "cocons_hip_glue.c")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # The ungrouped wrappers' argument lists are pinned (tests/test_vecchia_sim_abi.py, tests/test_vecchia_cv_abi.py), so the
    # switch is the shim: twin and grouped wrapper both call the one body `<twin>.by(shim, ...)`, which holds the only .Call
    cases = (("unwhiten", 3, "unwhiten", "fit, theta_list, W", "fit, theta_list, W"),
             ("sim", 5, "sim", "fit, theta_list, iiderrors, n_fixed = 0L, z_col = 1L", "fit, theta_list, iiderrors, n_fixed, z_col"),
             ("whiten_t", 3, "whiten.t", "fit, theta_list, W", "fit, theta_list, W"),
             ("cv", 3, "cv", "fit, theta_list, fold = NULL, safe = TRUE", "fit, theta_list, fold, safe"))
    for shim, arity, rname, params, passed in cases:
        plain, grouped = "_cocons_hip_vecchia_" + shim, "_cocons_hip_vecchia_" + shim + "_grouped"
        assert R.L.stub_registered_arity(grouped.encode()) == arity, grouped
        assert R.L.stub_registered_arity(plain.encode()) == arity, plain
        rx = r"\.cocons\.hip\.vecchia\." + rname.replace(".", r"\.")
        by = ".cocons.hip.vecchia." + rname + ".by("
        for wrapper, entry in ((rx + r"\.grouped", grouped), (rx, plain)):
            m = re.search(wrapper + r" <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
            assert m and m.group(1) == params, (rname, entry)
            assert m.group(2).strip().lstrip("{").strip() == by + "`%s`, " % entry + passed + ")", (rname, m.group(2))   # the call alone
        body = re.search(rx + r"\.by <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
        assert body and body.group(1) == "shim, " + passed and body.group(2).count(".Call(shim, ") == 1, rname
        assert src.count("`%s`" % grouped) == 1 and src.count("`%s`" % plain) == 1, rname    # no other path to either shim
        for name in (grouped, ".cocons.hip.vecchia." + rname + ".grouped"):
            assert name in doc, name
    for entry in (t + "_grouped" for t in TWINS):
        assert entry in glue, entry
        assert entry in doc, entry


def test_the_documents_name_the_entries_and_the_tool():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"^### 4ab\. ", design, re.M)
    for entry in [t + "_grouped" for t in TWINS] + [DEBUG, "launch_vecchia_group_coefs"]:
        assert entry in design, entry
    for entry in (t + "_grouped" for t in TWINS):
        assert entry in readme, entry
    assert "tools/vecchia_group_coef_timing.py" in readme and "tools/vecchia_group_coef_timing.py" in design
    assert "The grouped U⁻¹ and Uᵀ are the follow-ups." not in readme
    assert "tests/test_gpu_vecchia_group_coef.py" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "vecchia_group_coef_timing.py"))
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "VECCHIA_GROUP_COEF_REPORT.md"))


def test_host_layer_has_the_methods_and_the_pinned_signatures_stand():
    import cocons_amd as ca
    F = ca.CoconsVecchiaFit

    def params(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    # new
    assert params(F.unwhiten_grouped_core) == [("self", E), ("theta_list", E), ("W", E)]
    assert params(F.sim_grouped_core) == [("self", E), ("theta_list", E), ("iiderrors", E), ("n_fixed", 0), ("z_col", 0)]
    assert params(F.whiten_t_grouped_core) == [("self", E), ("theta_list", E), ("W", E)]
    assert params(F.cv_core)[-1] == ("grouped", False)
    assert params(ca.cocoSim_vecchia_grouped) == [("theta_list", E), ("locs", E), ("X_std", E), ("smooth_limits", E),
                                                  ("iiderrors", E), ("nn", None), ("m", None), ("max_rows", 64), ("fit", None)]
    assert params(ca.cocoCV_vecchia_grouped) == [("theta_list", E), ("locs", E), ("X_std", E), ("smooth_limits", E), ("z", E),
                                                 ("nn", None), ("m", None), ("fold", None), ("max_rows", 64), ("fit", None)]
    # pinned
    assert params(F.unwhiten_core) == params(F.unwhiten_grouped_core)
    assert params(F.sim_core) == params(F.sim_grouped_core)
    assert params(F.whiten_t_core) == params(F.whiten_t_grouped_core)
    assert params(F.cv_core)[:3] == [("self", E), ("theta_list", E), ("fold", None)]
    assert [k for k, _ in params(ca.cocoSim_vecchia)] == ["theta_list", "locs", "X_std", "smooth_limits", "iiderrors", "nn", "m", "fit"]
    assert [k for k, _ in params(ca.cocoCV_vecchia)] == ["theta_list", "locs", "X_std", "smooth_limits", "z", "nn", "m", "fold", "fit"]
    assert [k for k, _ in params(ca.cocoSim_cond_vecchia)] == ["theta_list", "locs", "newlocs", "X_std", "X_pred_std", "smooth_limits",
                                                               "z", "iiderrors", "m", "fit"]
    # without a table, a count or a fit the host forms refuse before any handle is made
    for fn, who in ((ca.cocoSim_vecchia_grouped, "cocoSim_vecchia_grouped"), (ca.cocoCV_vecchia_grouped, "cocoCV_vecchia_grouped")):
        with pytest.raises(ValueError, match=who):
            fn({}, np.zeros((3, 2)), np.zeros((3, 1)), (0.5, 2.5), np.zeros((3, 1)))
