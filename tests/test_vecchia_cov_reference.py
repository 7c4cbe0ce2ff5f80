"""The reference of U^-T on a Vecchia fit (tests/vecchia_cov_reference.py), without a GPU, pinned to a dense U built from the
coefficients on the oracle's matrices at n = 40 (test_gpu_dense_sizes.problem): U'(U^-T w) = w and U^-1 U^-T = (U'U)^-1 for
m = 5; with every predecessor in the table the model's covariance is Sigma(theta) itself and, for n_fixed = 24, the
conditional covariance is Sigma_pp - Sigma_po Sigma_oo^-1 Sigma_op; the largest transposed level is the largest forward level.

Bound of every comparison: PARITY = 1e-8 of test_gpu_dense_sizes, relative to the largest magnitude of the compared array.
The restatement in double differs from itself in long double by at most 4.7e-16 on these cases (printed below, recorded in
vecchia_cov_reference's docstring): the bound hides nothing of the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_cov_reference as VC  # noqa: E402
import vecchia_reference as VR  # noqa: E402
import vecchia_sim_reference as VS  # noqa: E402
from test_gpu_dense_sizes import PARITY, problem  # noqa: E402

N = 40


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _report(what, case, err):
    print("vecchia-cov-report reference | %s | %s | %.2e" % (what, case, err))


def _table(m):
    from cocons_amd import host
    return host.vecchia_neighbours(problem(N)[0], m).copy(order="F")


def test_recursion_against_the_dense_u_m5():
    S, nn = problem(N)[6], _table(5)
    coef = VS.coefficients(S, nn)
    U = VC.dense_u(coef, nn)
    W = np.random.default_rng(40).standard_normal((N, 3))
    v = VC.solve_t(coef, nn, W)
    errs = [_rel(U.T @ v, W), _rel(v, np.linalg.solve(U.T, W))]
    cov = VC.cov_mult(S, nn, np.eye(N), coef=coef)
    errs.append(_rel(cov, np.linalg.inv(U.T @ U)))
    errs.append(_rel(cov, np.linalg.inv(VR.precision_matrix(S, nn)[0])))
    # a fixed part: the block of U behind it
    nf = 13
    Upp = U[nf:, nf:]
    errs.append(_rel(VC.solve_t(coef, nn, W[nf:], nf), np.linalg.solve(Upp.T, W[nf:])))
    errs.append(_rel(VC.cov_mult(S, nn, np.eye(N - nf), nf, coef=coef), np.linalg.inv(Upp.T @ Upp)))
    _report("U'(U^-T w) = w, solve(U', w), (U'U)^-1, fixed 13", "n40 m5", max(errs))
    assert max(errs) < PARITY, errs


def test_all_predecessors_is_sigma_and_the_conditional_covariance():
    S = problem(N)[6]
    nn = VR.all_predecessors(N)
    coef = VS.coefficients(S, nn)
    cov = VC.cov_mult(S, nn, np.eye(N), coef=coef)
    err = _rel(cov, S)
    _report("Sigma~ = Sigma", "n40 m39", err)
    assert err < PARITY, err
    nf = 24
    cond = S[nf:, nf:] - S[nf:, :nf] @ np.linalg.solve(S[:nf, :nf], S[:nf, nf:])
    got = VC.cov_mult(S, nn, np.eye(N - nf), nf, coef=coef)
    err = _rel(got, cond)
    _report("Cov(p | o) = S_pp - S_po S_oo^-1 S_op", "n40 m39 fixed 24", err)
    assert err < PARITY, err


@pytest.mark.parametrize("m", (1, 5, 39))
def test_tlevels(m):
    nn = VR.all_predecessors(N) if m == 39 else _table(m)
    for nf in (0, 1, 17, N - 1):
        tl, fl = VC.tlevels(nn, nf), VS.levels(nn, nf)
        assert tl.dtype == np.int32 and np.all(tl[:nf] == 0) and np.all(tl[nf:] >= 1)
        assert tl.max() == fl.max(), (m, nf)                 # the same longest path
        lists = VC.named_by(nn)
        for j in range(nf, N):
            assert tl[j] == 1 + max((tl[k] for k, _ in lists[j]), default=0)
    chain = np.zeros((N, 1), dtype=np.int32)
    chain[1:, 0] = np.arange(1, N)
    assert np.array_equal(VC.tlevels(chain), np.arange(N, 0, -1))
    star = np.zeros((N, 1), dtype=np.int32)
    star[1:, 0] = 1
    assert np.array_equal(VC.tlevels(star), np.concatenate([[2], np.ones(N - 1)]))
    assert np.array_equal(VC.tlevels(star, 1), np.concatenate([[0], np.ones(N - 1)]))


def test_double_against_long_double():
    S = problem(N)[6]
    W = np.random.default_rng(41).standard_normal((N, 3))
    worst = 0.0
    for m, nf in ((5, 0), (5, 13), (39, 24)):
        nn = VR.all_predecessors(N) if m == 39 else _table(m)
        cd, cl = VS.coefficients(S, nn), VS.coefficients(S, nn, np.longdouble)
        for what, fn in (("unwhiten_t", VC.solve_t), ("cov_mult", lambda c, t, w, f: VC.solve(c, t, VC.solve_t(c, t, w, f), f))):
            err = _rel(fn(cd, nn, W[nf:], nf), np.asarray(fn(cl, nn, W[nf:], nf), dtype=float))
            _report("double against long double, %s" % what, "n40 m%d fixed %d" % (m, nf), err)
            worst = max(worst, err)
    assert worst < 1e-12, worst
