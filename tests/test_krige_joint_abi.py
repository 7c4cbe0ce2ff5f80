"""Joint prediction from the held factor at the boundary, without a GPU: the C ABI declares and exports
cocons_krige_joint, the ctypes binding carries it with its 10 arguments, every refusal that needs no handle returns -1 with
a message naming the entry point before any HIP call and leaves the outputs alone, the R glue registers
_cocons_hip_krige_joint with arity 6, the R wrapper calls it and INTEGRATION.md names it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int\s+cocons_krige_joint\s*\(\s*cocons_fit\s*\*\s*fit,\s*int m,\s*const double \*locs_pred,\s*"
        r"const double \*X_pred,\s*const double \*locs_unobs,[^;]*?double \*stochastic,[^;]*?double \*cov,[^;]*?"
        r"int nsim,\s*const double \*iiderrors,[^;]*?double \*sims\s*\)\s*;")


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    assert re.search(DECL, h)
    assert len(_lib.SIGNATURES["cocons_krige_joint"][1]) == 10
    L = _lib.load()
    assert hasattr(L, "cocons_krige_joint")
    assert L.cocons_abi_version() == 1
    import cocons_amd as ca
    for name in ("cocoPredict_dense_joint", "cocoSim_cond_dense_held"):
        assert callable(getattr(ca, name))
    assert callable(ca.CoconsFit.krige_joint_core)


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    m, p, nsim = 3, 3, 2
    lp, Xp, lu = np.zeros(m * 2), np.zeros(m * p), np.zeros(m * 2)
    E = np.zeros(m * nsim)
    st, cov, sims = np.full(m, 7.0), np.full(m * m, 7.0), np.full(m * nsim, 7.0)
    J = L.cocons_krige_joint
    cases = {
        "null handle": lambda: J(None, m, _dp(lp), _dp(Xp), _dp(lu), _dp(st), _dp(cov), nsim, _dp(E), _dp(sims)),
        "m = 0": lambda: J(None, 0, _dp(lp), _dp(Xp), _dp(lu), _dp(st), _dp(cov), nsim, _dp(E), _dp(sims)),
        "m < 0": lambda: J(None, -2, _dp(lp), _dp(Xp), _dp(lu), _dp(st), _dp(cov), nsim, _dp(E), _dp(sims)),
        "null locs_pred": lambda: J(None, m, None, _dp(Xp), _dp(lu), _dp(st), _dp(cov), nsim, _dp(E), _dp(sims)),
        "null X_pred": lambda: J(None, m, _dp(lp), None, _dp(lu), _dp(st), _dp(cov), nsim, _dp(E), _dp(sims)),
        "null stochastic": lambda: J(None, m, _dp(lp), _dp(Xp), _dp(lu), None, _dp(cov), nsim, _dp(E), _dp(sims)),
        "nsim < 0": lambda: J(None, m, _dp(lp), _dp(Xp), _dp(lu), _dp(st), _dp(cov), -1, _dp(E), _dp(sims)),
        "null iiderrors": lambda: J(None, m, _dp(lp), _dp(Xp), _dp(lu), _dp(st), _dp(cov), nsim, None, _dp(sims)),
        "null sims": lambda: J(None, m, _dp(lp), _dp(Xp), _dp(lu), _dp(st), _dp(cov), nsim, _dp(E), None),
    }
    for what, call in cases.items():
        assert call() == -1, what
        msg = _lib.last_error()
        assert msg.startswith("cocons_krige_joint:"), (what, msg)
        if what == "null handle":
            assert "null fit handle" in msg
    assert np.all(st == 7.0) and np.all(cov == 7.0) and np.all(sims == 7.0)


def test_glue_registers_the_entry_and_the_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_krige_joint") == 6
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.krige\.joint <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_krige_joint`" in m.group(2)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_krige_joint", "_cocons_hip_krige_joint", ".cocons.hip.krige.joint"):
        assert entry in doc
