"""The numpy statement of the Vecchia fit's expected information (tests/vecchia_fisher_reference.py) checked against itself and
against the dense statement, and cocons_fisher_vecchia at the boundary, all without a GPU: declared, bound, exported, bad calls
refused with -1 and a message naming the entry before any HIP call (outputs untouched), the R glue registered."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
import vecchia_fisher_reference as VF  # noqa: E402
import vecchia_reference as VR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = np.eye(18).reshape(18, 6, 3)
DIRS = np.concatenate([UNITS, FR.scaling_direction(3)[None]])      # the 6 p unit tables, then the scaling direction

DECL = (r"int\s+cocons_fisher_vecchia\s*\(\s*cocons_fit\s*\*\s*fit,\s*const double \*theta,\s*int ndir,\s*const double \*dirs,\s*"
        r"double \*info,\s*double \*info_mean\s*\)\s*;")


@functools.lru_cache(maxsize=None)
def _matrices(n):
    from cocons_amd import host, workloads as wl
    locs, X, th = VF.setup(n)
    S, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, DIRS)
    S.setflags(write=False)
    Sa.setflags(write=False)
    return locs, X, S, Sa


def _table(n, m):
    from cocons_amd import host
    return host.vecchia_neighbours(_matrices(n)[0], m)


def test_the_dense_statement_orients_coincident_pairs_as_the_block_kernel_does():
    """a coincident pair's entry of Sigma_a is the EARLIER site's diagonal partial, whichever way the pair is read"""
    from cocons_amd import host, workloads as wl
    locs, X, th = VF.setup(12)
    locs[9] = locs[4]
    S, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, DIRS)
    assert S[9, 4] == S[4, 4] and S[4, 9] == S[4, 4] and S[9, 9] != S[4, 4]
    assert np.array_equal(Sa[:, 9, 4], Sa[:, 4, 4]) and np.array_equal(Sa[:, 4, 9], Sa[:, 4, 4])


@pytest.mark.parametrize("n,m", ((150, 10), (150, 30), (65, 63)))
def test_the_two_statements_agree(n, m):
    locs, X, S, Sa = _matrices(n)
    nn = _table(n, m)
    a = VF.info_blocks(S, Sa, nn, 2)
    b, _ = VF.info_last_row(S, Sa, nn, 2)
    print("vecchia-fisher-report cpu | last-row statement vs block difference (metric) | n%d m%d | %.2e" % (n, m, FR.metric(b, a)))
    assert FR.metric(b, a) <= 1e-12


def test_exact_with_all_predecessors():
    n = 64
    locs, X, S, Sa = _matrices(n)
    nn = VR.all_predecessors(n)
    want = FR.info_solve(S, Sa, 1)
    got, gm = VF.info_last_row(S, Sa, nn, 1, X)
    print("vecchia-fisher-report cpu | all predecessors vs FR.info_solve, last row and block difference (metric) | n64 | "
          "%.2e %.2e" % (FR.metric(got, want), FR.metric(VF.info_blocks(S, Sa, nn), want)))
    assert FR.metric(got, want) <= 1e-12 and FR.metric(VF.info_blocks(S, Sa, nn), want) <= 1e-12
    wm = X.T @ np.linalg.solve(S, X)
    assert np.max(np.abs(gm - wm)) <= 1e-10 * np.max(np.abs(wm))


@pytest.mark.parametrize("m", (10, 30))
def test_the_table_matters(m):
    """nothing that ignores the table can pass: the gap to the dense information is far above every bound used on the GPU"""
    n = 150
    locs, X, S, Sa = _matrices(n)
    got, _ = VF.info_last_row(S, Sa, _table(n, m))
    gap = FR.metric(got, FR.info_solve(S, Sa, 1))
    print("vecchia-fisher-report cpu | distance from the dense information, must exceed 1e-3 (metric) | n%d m%d | %.2e" % (n, m, gap))
    assert gap > 1e-3


@pytest.mark.parametrize("n,m,r", ((150, 10, 1), (150, 30, 3), (65, 63, 2), (1, 1, 1)))
def test_scaling_direction_and_semidefiniteness(n, m, r):
    locs, X, S, Sa = _matrices(n)
    nn = _table(n, m)
    nn = nn.copy(order="F")
    nn[::3, 0] = 0                                  # any table
    info, _ = VF.info_last_row(S, Sa, nn, r)
    assert abs(info[18, 18] - r * n / 2) <= 1e-12 * r * n
    ev = np.linalg.eigvalsh(info)
    assert ev[0] >= -1e-12 * ev[-1]


def _dp(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


def test_declared_bound_exported():
    from cocons_amd import _lib
    L = _lib.load()
    assert re.search(DECL, open(os.path.join(ROOT, "include", "cocons_hip.h")).read())
    assert "cocons_fisher_vecchia" in _lib.SIGNATURES and len(_lib.SIGNATURES["cocons_fisher_vecchia"][1]) == 6
    assert hasattr(L, "cocons_fisher_vecchia")


def test_bad_calls_are_refused_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    p = 3
    th, dirs = np.zeros(6 * p), np.ones((2, 6 * p))
    info, im = np.full(4, 7.0), np.full(p * p, 7.0)
    assert L.cocons_fisher_vecchia(None, _dp(th), 2, _dp(dirs), _dp(info), _dp(im)) == -1
    msg = _lib.last_error()
    assert msg.startswith("cocons_fisher_vecchia:") and "null fit handle" in msg, msg
    bogus = ctypes.c_void_p(0x1000)        # never dereferenced: the arguments are checked first
    for args in ((None, _dp(dirs), _dp(info)), (_dp(th), None, _dp(info)), (_dp(th), _dp(dirs), None)):
        assert L.cocons_fisher_vecchia(bogus, args[0], 2, args[1], args[2], _dp(im)) == -1
        assert _lib.last_error().startswith("cocons_fisher_vecchia: null argument")
    for nd in (0, -1, 7 * _lib.P_MAX + 1):
        assert L.cocons_fisher_vecchia(bogus, _dp(th), nd, _dp(dirs), _dp(info), _dp(im)) == -1
        msg = _lib.last_error()
        assert msg.startswith("cocons_fisher_vecchia:") and "ndir" in msg, msg
    assert np.all(info == 7.0) and np.all(im == 7.0)


def test_glue_registers_the_entry_and_the_r_wrapper_calls_it():
    from test_glue_exec import RStub
    R = RStub()
    assert R.L.stub_registered_arity(b"_cocons_hip_vecchia_fisher") == 3
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    body = src[src.index(".cocons.hip.vecchia.fisher <- function"):]
    assert "`_cocons_hip_vecchia_fisher`" in body[:body.index("\n}\n")]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ("cocons_fisher_vecchia", ".cocons.hip.vecchia.fisher", "getFisher_vecchia"):
        assert entry in doc
    import cocons_amd as ca
    assert callable(ca.getFisher_vecchia) and callable(ca.CoconsVecchiaFit.fisher_core)
