"""The grouped Vecchia gradient at the boundary, without a GPU, in the pattern of tests/test_vecchia_cv_abi.py:
the header declares cocons_neg2loglik_grad_vecchia_grouped with the ungrouped entry's argument list, the library exports it
(nm -D) and the ctypes binding carries it; every call that can be refused on its arguments alone is refused with -1 and a
message that starts with the entry's name, before any HIP call, with the outputs untouched; the R glue registers its shim with
its arity and the R wrapper names it; the documents name the entry; and the host layer takes the keyword.  (The refusals that
need a handle -- no plan, another kind of handle -- are in tests/test_gpu_vecchia_group_grad.py.)"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cocons_neg2loglik_grad_vecchia_grouped"
ARGS = (r"\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*const double \*mean,\s*int c,\s*const double \*B,\s*"
        r"double \*sum_logliks,\s*double \*parts,\s*double \*grad_theta,\s*double \*grad_quad,\s*double \*grad_mean\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"int\s+" + ENTRY + ARGS, h, re.S)
    assert re.search(r"int\s+cocons_neg2loglik_grad_vecchia" + ARGS, h, re.S)      # the same argument list
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["cocons_neg2loglik_grad_vecchia"] and len(_lib.SIGNATURES[ENTRY][1]) == 10
    assert hasattr(L, ENTRY)
    assert re.search(r" T %s$" % ENTRY, exported, re.M)
    assert L.cocons_abi_version() == 1
    for text in (r"agrees with cocons_neg2loglik_grad_vecchia on the same handle to\s*\*?\s*rounding, not to the bit",
                 r"a handle without\s*\*?\s*a plan"):
        assert re.search(text, h), text


def test_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p, n, c = 2, 5, 2
    theta, mean, B = np.zeros(6 * p), np.zeros(p), np.ones(n * c)
    val = np.full(1, 7.0)
    parts, gt, gq, gm = np.full(1 + c, 7.0), np.full(6 * p, 7.0), np.full(6 * p, 7.0), np.full(p, 7.0)
    fake = ctypes.c_void_p(1)           # never dereferenced: every case below is refused on its arguments alone

    def call(f=fake, theta_=theta, mean_=mean, c_=0, B_=None, val_=val, gt_=gt, gm_=gm):
        return getattr(L, ENTRY)(f, _dp(theta_), _dp(mean_), c_, _dp(B_), _dp(val_), _dp(parts), _dp(gt_), _dp(gq), _dp(gm_))

    assert call(f=None) == -1
    assert _lib.last_error() == ENTRY + ": null fit handle"
    for kw in (dict(theta_=None), dict(val_=None), dict(gt_=None), dict(mean_=None), dict(gm_=None)):
        assert call(**kw) == -1, kw
        assert _lib.last_error() == ENTRY + ": null argument", kw
    for kw in (dict(B_=B, c_=c), dict(B_=B, c_=c, mean_=None), dict(B_=B, c_=c, gm_=None)):      # B together with mean
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith(ENTRY + ": B is given, so mean and grad_mean must be NULL"), kw
    for bad in (0, -2):
        assert call(B_=B, c_=bad, mean_=None, gm_=None) == -1
        assert _lib.last_error() == ENTRY + ": c = %d (at least one column expected)" % bad
    for a in (val, parts, gt, gq, gm):
        assert np.all(a == 7.0)


def test_glue_registers_the_shim_and_the_r_wrapper_exists():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_vecchia_neg2loglik_grad_grouped") == 3
    assert R.L.stub_registered_arity(b"_cocons_hip_vecchia_neg2loglik_grad") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.vecchia\.neg2loglik\.grad\.grouped <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_vecchia_neg2loglik_grad_grouped`" in m.group(2)
    assert m.group(1) == "fit, theta_list, safe = TRUE"
    glue = open(os.path.join(ROOT, "glue", "cocons_hip_glue.c")).read()
    assert ENTRY in glue
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in (ENTRY, "_cocons_hip_vecchia_neg2loglik_grad_grouped", ".cocons.hip.vecchia.neg2loglik.grad.grouped"):
        assert entry in doc, entry
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^### 4z\. ", design, re.M) and ENTRY in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert ENTRY in readme and "tools/vecchia_group_grad_timing.py" in readme


def test_host_layer_takes_the_keyword():
    import cocons_amd as ca
    sig = inspect.signature(ca.CoconsVecchiaFit.neg2loglik_grad_core)
    assert list(sig.parameters)[1:] == ["theta_list", "B", "grouped"]
    assert sig.parameters["B"].default is None and sig.parameters["grouped"].default is False
    for fn in (ca.GetNeg2loglikelihoodVecchia_grad, ca.GetNeg2loglikelihoodVecchiaProfile_grad, ca.GetNeg2loglikelihoodVecchiaREML_grad):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["fit", "grouped"] and params["grouped"].default is False, fn.__name__
    # the value forms keep theirs
    assert inspect.signature(ca.CoconsVecchiaFit.neg2loglik_core).parameters["grouped"].default is False
