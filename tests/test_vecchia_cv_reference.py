"""The reference of U' and of cross-validation on a Vecchia fit (tests/vecchia_cv_reference.py), without a GPU: against brute
force that shares none of its code, against Sigma(theta) itself where the Vecchia model is exact, its transposed lists against
a dictionary built row by row, and float64 against long double on every case tests/test_gpu_vecchia_cv.py uses.

Bounds.  BRUTE = 1e-9 relative to the largest magnitude of the compared array: the brute force inverts Q = U'U (cond(Q) =
cond(U)^2 <= 4096 on these cases, tests/golden/VECCHIA_SIM_REPORT.md) and solves with a block of the inverse, whose condition
is at most cond(Q) again; n <= 300, so about eps n cond(Q) = 2.2e-16 * 300 * 4096 = 2.7e-10.  LONG = 1e-11: the issue asks that
the reference's own float64 - long-double gap stands at least three orders below PARITY = 1e-8."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_reference as VR  # noqa: E402
import vecchia_cv_reference as VC  # noqa: E402
from test_gpu_dense_sizes import PARITY, problem  # noqa: E402

BRUTE = 1e-9
LONG = 1e-11
assert LONG <= PARITY * 1e-3


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _report(what, case, err):
    print("vecchia-cv-report reference | %s | %s | %.2e" % (what, case, err))


def _brute(Sv, R, fold):
    """resid_B = R_B - Sv_BA Sv_AA^-1 R_A, var = diag(Sv_BB - Sv_BA Sv_AA^-1 Sv_AB), label by label"""
    n = Sv.shape[0]
    resid, var = np.zeros(R.shape), np.zeros(n)
    for lab in np.unique(fold):
        B, A = np.nonzero(fold == lab)[0], np.nonzero(fold != lab)[0]
        if A.size == 0:
            resid[B], var[B] = R[B], np.diag(Sv)[B]
            continue
        G = np.linalg.solve(Sv[np.ix_(A, A)], np.column_stack([R[A], Sv[np.ix_(A, B)]]))
        resid[B] = R[B] - Sv[np.ix_(B, A)] @ G[:, :R.shape[1]]
        var[B] = np.diag(Sv[np.ix_(B, B)] - Sv[np.ix_(B, A)] @ G[:, R.shape[1]:])
    return resid, var


@pytest.mark.parametrize("spec", ((65, 10), (65, 10, True), (300, 30), (300, 30, True), (2, 1)), ids=str)
def test_against_brute_force_on_the_model_covariance(spec):
    """Sigma_v = (U'U)^-1 with U from vecchia_reference.precision_matrix (the blocks' inverse factors, not the coefficients the
    reference solves for)"""
    c = VC.case(spec)
    n = c["nn"].shape[0]
    Ub = VR.precision_matrix(c["S"], c["nn"])[1]
    Sv = np.linalg.inv(Ub.T @ Ub)
    errs = []
    got = VC.loo(c["U"], c["R"])
    want = _brute(Sv, c["R"], np.arange(n))
    errs += [_rel(got[0], want[0]), _rel(got[1], want[1])]
    lays = VC.layouts(n, c["locs"]) if n >= 300 else {"halves": (np.arange(n) % 2).astype(np.int32)} if n > 2 else {}
    for name, fold in lays.items():
        got = VC.folds(c["U"], c["R"], fold, c["Q"])
        want = _brute(Sv, c["R"], fold)
        errs += [_rel(got[0], want[0]), _rel(got[1], want[1])]
    W = np.random.default_rng(n).standard_normal((n, 3))
    ut, qd = VC.whiten_t(c["U"], W)
    errs += [_rel(ut, Ub.T @ W), _rel(qd, np.diag(Ub.T @ Ub)), _rel(c["Q"], Ub.T @ Ub)]
    _report("loo, folds, whiten_t against brute force", str(spec), max(errs))
    assert max(errs) < BRUTE, errs


def test_exact_when_every_predecessor_is_named():
    """n = 64, m = 63: the Vecchia model is Sigma(theta) itself"""
    n = 64
    locs, X, th, z = problem(65)[:4]
    S = problem(65)[6][:n, :n]
    R = (np.asarray(z) - (np.asarray(X) @ th["mean"])[:, None])[:n]
    U = VC.dense_u(S, VR.all_predecessors(n))
    fold = (np.arange(n) % 5).astype(np.int32)
    errs = []
    for got, want in ((VC.loo(U, R), _brute(S, R, np.arange(n))), (VC.folds(U, R, fold), _brute(S, R, fold))):
        errs += [_rel(got[0], want[0]), _rel(got[1], want[1])]
    errs.append(_rel(np.linalg.inv(VC.precision(U)), S))
    _report("exact: Sigma itself", "n64 m63", max(errs))
    assert max(errs) < BRUTE, errs


@pytest.mark.parametrize("spec", ((65, 10, True), (300, 30), "wide", "zero", (1, 1)), ids=str)
def test_transposed_lists_against_a_dictionary(spec):
    nn = VC.case(spec)["nn"] if not isinstance(spec, str) else __import__("test_gpu_vecchia_sim").special(spec)
    n = nn.shape[0]
    lists = {j: [] for j in range(n)}
    for i in range(n):
        for v in nn[i]:
            if v > 0:
                lists[int(v) - 1].append(i + 1)
    ptr, rows = VC.transpose(nn)
    assert ptr.dtype == np.int32 and rows.dtype == np.int32 and ptr[0] == 0 and ptr[n] == rows.size == int(np.sum(nn > 0))
    for j in range(n):
        assert list(rows[ptr[j]:ptr[j + 1]]) == sorted(lists[j])
        assert all(k > j + 1 for k in lists[j])
    if spec == "wide":
        assert int(np.max(np.diff(ptr))) == 577 + 1           # the 577 late rows and row 2 name row 1


@pytest.mark.parametrize("spec", VC.SPECS, ids=str)
def test_float64_against_long_double_on_the_gpu_cases(spec):
    c = VC.case(spec)
    n = c["nn"].shape[0]
    Ul = VC.dense_u(c["S"], c["nn"], long_double=True)
    W = np.random.default_rng(1000 + n).standard_normal((n, 3))
    errs = []
    for a, b in zip(VC.whiten_t(c["U"], W) + VC.loo(c["U"], c["R"]), VC.whiten_t(Ul, W) + VC.loo(Ul, c["R"])):
        errs.append(_rel(a, b))
    if spec in VC.FOLD_SPECS:
        Ql = VC.precision(Ul)
        for name, fold in VC.layouts(n, c["locs"]).items():
            for a, b in zip(VC.folds(c["U"], c["R"], fold, c["Q"]), VC.folds(Ul, c["R"], fold, Ql)):
                errs.append(_rel(a, b))
    _report("float64 against long double", str(spec), max(errs))
    assert max(errs) < LONG, errs
