"""The grouped Vecchia information at the boundary, without a GPU, in the pattern of
tests/test_vecchia_group_grad_abi.py: the header declares cocons_fisher_vecchia_grouped with the ungrouped entry's argument
list, the library exports it (nm -D) and the ctypes binding carries it; every call that can be refused on its arguments alone
is refused with -1 and a message that starts with the entry's name, before any HIP call, with the outputs untouched; the R glue
registers its shim with its arity and the R wrapper names it; the documents name the entry; and the host layer takes the
keyword.  (The refusals that need a handle -- no plan, another kind of handle, non-finite directions, which are checked behind
the handle's kind -- are in tests/test_gpu_vecchia_group_fisher.py.)"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cocons_fisher_vecchia_grouped"
ARGS = (r"\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int ndir,\s*const double \*dirs,\s*"
        r"double \*info,\s*double \*info_mean\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_dp)


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"int\s+" + ENTRY + ARGS, h, re.S)
    assert re.search(r"int\s+cocons_fisher_vecchia" + ARGS, h, re.S)      # the same argument list
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["cocons_fisher_vecchia"] and len(_lib.SIGNATURES[ENTRY][1]) == 6
    assert hasattr(L, ENTRY)
    assert re.search(r" T %s$" % ENTRY, exported, re.M)
    assert L.cocons_abi_version() == 1
    for text in (r"agrees with\s*\*?\s*cocons_fisher_vecchia on the same handle to rounding, not to the bit",
                 r"a handle without\s*\*?\s*a plan"):
        assert re.search(text, h), text


def test_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p = 3
    theta, dirs = np.zeros(6 * p), np.ones((2, 6 * p))
    info, im = np.full(4, 7.0), np.full(p * p, 7.0)
    fake = ctypes.c_void_p(1)           # never dereferenced: every case below is refused on its arguments alone

    def call(f=fake, theta_=theta, nd=2, dirs_=dirs, info_=info):
        return getattr(L, ENTRY)(f, _dp(theta_), nd, _dp(dirs_), _dp(info_), _dp(im))

    assert call(f=None) == -1
    assert _lib.last_error() == ENTRY + ": null fit handle"
    for kw in (dict(theta_=None), dict(dirs_=None), dict(info_=None)):
        assert call(**kw) == -1, kw
        assert _lib.last_error() == ENTRY + ": null argument", kw
    for nd in (0, -1, 7 * _lib.P_MAX + 1):
        assert call(nd=nd) == -1
        assert _lib.last_error() == ENTRY + ": ndir = %d is outside [1, %d]" % (nd, 7 * _lib.P_MAX)
    assert np.all(info == 7.0) and np.all(im == 7.0)


def test_glue_registers_the_shim_and_the_r_wrapper_exists():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_vecchia_fisher_grouped") == 3
    assert R.L.stub_registered_arity(b"_cocons_hip_vecchia_fisher") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.vecchia\.fisher\.grouped <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and m.group(1) == "fit, theta, par.pos, safe = TRUE"
    assert ".cocons.hip.vecchia.fisher(fit, theta, par.pos, safe, grouped = TRUE)" in m.group(2)      # one Jacobian code
    shared = re.search(r"\.cocons\.hip\.vecchia\.fisher <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert shared and "`_cocons_hip_vecchia_fisher_grouped`" in shared.group(2) and "`_cocons_hip_vecchia_fisher`" in shared.group(2)
    glue = open(os.path.join(ROOT, "glue", "cocons_hip_glue.c")).read()
    assert ENTRY in glue
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in (ENTRY, "_cocons_hip_vecchia_fisher_grouped", ".cocons.hip.vecchia.fisher.grouped"):
        assert entry in doc, entry
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^### 4aa\. ", design, re.M) and ENTRY in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert ENTRY in readme and "tools/vecchia_group_fisher_timing.py" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "vecchia_group_fisher_timing.py"))


def test_host_layer_takes_the_keyword():
    import cocons_amd as ca
    sig = inspect.signature(ca.CoconsVecchiaFit.fisher_core)
    assert list(sig.parameters)[1:] == ["theta_list", "dirs", "grouped"] and sig.parameters["grouped"].default is False
    params = inspect.signature(ca.getFisher_vecchia).parameters
    assert list(params)[-2:] == ["fit", "grouped"] and params["grouped"].default is False
