"""The expected information of a tapered fit at the boundary, without a GPU: cocons_fisher_taper is declared, bound and
exported, bad calls are refused with -1 and a message naming the entry before any HIP call (outputs untouched), the R glue
registers the entry with its arity, the R wrapper calls it, and the host layer offers it."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int\s+cocons_fisher_taper\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int ndir,\s*const double \*dirs,\s*"
        r"int nprobe,\s*const double \*probes,\s*int max_rows,\s*double \*info,\s*double \*info_mean\s*\)\s*;")


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    assert re.search(DECL, open(os.path.join(ROOT, "include", "cocons_hip.h")).read())
    assert "cocons_fisher_taper" in _lib.SIGNATURES and len(_lib.SIGNATURES["cocons_fisher_taper"][1]) == 9
    assert hasattr(L, "cocons_fisher_taper")
    assert L.cocons_abi_version() == 1


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p, n = 3, 10
    th, dirs, probes = np.zeros(6 * p), np.ones((2, 6 * p)), np.ones((n, 4))
    info, im = np.full(4, 7.0), np.full(p * p, 7.0)
    assert L.cocons_fisher_taper(None, _dp(th), 2, _dp(dirs), 0, None, 0, _dp(info), _dp(im)) == -1
    msg = _lib.last_error()
    assert msg.startswith("cocons_fisher_taper:") and "null fit handle" in msg, msg
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the arguments are checked first
    for args in ((None, _dp(dirs), _dp(info)), (_dp(th), None, _dp(info)), (_dp(th), _dp(dirs), None)):
        assert L.cocons_fisher_taper(bogus, args[0], 2, args[1], 0, None, 0, args[2], _dp(im)) == -1
        assert _lib.last_error().startswith("cocons_fisher_taper: null argument")
    for nd in (0, -1, 7 * _lib.P_MAX + 1):
        assert L.cocons_fisher_taper(bogus, _dp(th), nd, _dp(dirs), 0, None, 0, _dp(info), _dp(im)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_fisher_taper:") and "ndir" in msg, msg
    for nprobe, pr in ((-1, None), (-1, _dp(probes)), (4, None), (0, _dp(probes))):
        assert L.cocons_fisher_taper(bogus, _dp(th), 2, _dp(dirs), nprobe, pr, 0, _dp(info), _dp(im)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_fisher_taper:") and "nprobe" in msg, msg
    for nprobe, pr in ((0, None), (4, _dp(probes))):
        assert L.cocons_fisher_taper(bogus, _dp(th), 2, _dp(dirs), nprobe, pr, -64, _dp(info), _dp(im)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_fisher_taper:") and "max_rows" in msg, msg
    assert np.all(info == 7.0) and np.all(im == 7.0)


def test_glue_registers_the_entry_and_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_fisher_taper") == 5
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    m = re.search(r"\.cocons\.hip\.fisher\.taper <- function\(([^)]*)\)(.*?)\n(?=\S|$)", src, re.S)
    assert m and "`_cocons_hip_fisher_taper`" in m.group(2) and "nprobe" in m.group(1)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_fisher_taper", ".cocons.hip.fisher.taper"):
        assert entry in doc


def test_host_layer_offers_it():
    import inspect
    import cocons_amd as ca
    from cocons_amd import host
    assert ca.getFisher_sparse is host.getFisher_sparse
    sig = inspect.signature(host.getFisher_sparse)
    assert list(sig.parameters)[:8] == ["par", "par_pos", "locs", "x_covariates", "smooth_limits", "z", "n", "ref_taper"]
    assert sig.parameters["nprobe"].default == 0 and sig.parameters["seed"].default == 0 and "fit" in sig.parameters
    doc = host.getFisher_sparse.__doc__
    assert "nprobe = 0" in doc and "exact" in doc and "n^2" in doc
    core = inspect.signature(host.CoconsTaperFit.fisher_core)
    assert list(core.parameters) == ["self", "theta_list", "dirs", "probes", "max_rows"]
    assert host.CoconsTaperFit.fisher_core is not host.CoconsFit.fisher_core
