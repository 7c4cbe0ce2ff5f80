"""tests/conditioning_cases.py on the CPU, on the oracle's Sigma alone: the cases are as ill-conditioned as their table says,
still positive definite with room to spare, and 1e3 x harder for LAPACK than the benign case every other test uses -- so an
edit of theta that makes them easy again fails here, not silently in the GPU tests."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_cases as cc  # noqa: E402


@functools.lru_cache(maxsize=None)
def _sigma(case, gx, gy):
    from oracle import oracle as O
    pb = cc.problem(case, gx, gy)
    return pb, O.cov_rns(pb.theta, pb.locs, pb.X, pb.smooth_limits)


@functools.lru_cache(maxsize=None)
def _relative_yardstick(case, gx, gy):
    """LAPACK's six-ordering error relative to the reference, per quantity (logdet, quad of either realisation);
    raises if LAPACK or chol_ld finds the matrix not positive definite in any ordering."""
    pb, S = _sigma(case, gx, gy)
    v = cc.referee(S, cc.residual(pb))
    return np.r_[v.yard["logdet"] / abs(v.ref["logdet"]), v.yard["quad"] / np.abs(v.ref["quad"])]


@pytest.mark.parametrize("case,gx,gy", cc.CASE_SIZES)
def test_condition_number_and_margin(oracle, case, gx, gy):
    """cond(Sigma) in its stated decade; lambda_min / lambda_max >= 50 n 2^-53, the distance from a legitimate "not positive
    definite" (case B at n = 841 would have 17 n 2^-53 and is left out)."""
    pb, S = _sigma(case, gx, gy)
    w = np.linalg.eigvalsh(S)
    cond = w[-1] / w[0]
    lo, hi = cc.CASES[case].cond[(gx, gy)]
    assert lo <= cond < hi, (case, pb.n, cond)
    assert w[0] / w[-1] >= 50 * pb.n * 2.0 ** -53, (case, pb.n, w[0] / w[-1] / (pb.n * 2.0 ** -53))


@pytest.mark.parametrize("case,gx,gy", cc.CASE_SIZES)
def test_positive_definite_and_hard(oracle, case, gx, gy):
    """LAPACK factors all six orderings and chol_ld returns info 0 (referee raises otherwise); the yardstick of A .. D is
    at least 1e3 x the base case's at the same size, quantity by quantity."""
    y = _relative_yardstick(case, gx, gy)
    assert np.all(np.isfinite(y))
    if case in cc.HARD:
        base = _relative_yardstick("base", gx, gy)
        assert np.all(y >= 1e3 * base), (case, y, base)


@pytest.mark.parametrize("case", list(cc.CASES))
def test_the_measure_sees_a_backward_error_of_1e_minus_12(oracle, case):
    """How sharp the measure is: Sigma with every entry off by up to 2^-40 relative (9e-13, symmetric, unstructured -- what
    a sloppy trailing update or panel solve would leave behind, and a hundred times below the tightest tolerance of the
    other parity tests), factored by LAPACK and judged like a device path.  On A .. D the log-determinant and the white-noise
    quadratic form miss the bound (ratios 50 .. 1000 over three seeds when this was written, 10 allowed); on the benign case
    the same perturbation passes unnoticed, which is why these cases exist."""
    pb, S = _sigma(case, 25, 25)
    S = cc.sym(S)
    B = cc.residual(pb)
    v = cc.referee(S, B)
    U = np.tril(np.random.default_rng(0).uniform(-1, 1, S.shape))
    L, Y = cc.lapack_solve(S * (1 + np.ldexp(U + np.tril(U, -1).T, -40)), B)
    r_ld = cc.ratio(np.sum(np.log(np.diag(L))), v.yard["logdet"], v.ref["logdet"])
    r_q0 = cc.ratio(np.sum(Y[:, 0] ** 2), v.yard["quad"][0], v.ref["quad"][0])
    if case in cc.HARD:
        assert r_ld > cc.FACTOR and r_q0 > cc.FACTOR, (case, r_ld, r_q0)
    else:
        assert r_ld <= cc.FACTOR and r_q0 <= cc.FACTOR, (case, r_ld, r_q0)


def test_case_table_is_the_issue_s():
    """Sizes, tile counts and what is left out: 14 (case, size) pairs, n > 512 everywhere (the engine and the persistent
    launch need more than four tiles), case B not at n = 841."""
    assert len(cc.CASE_SIZES) == 14 and ("B", 29, 29) not in cc.CASE_SIZES
    assert [gx * gy for gx, gy in cc.SIZES] == [625, 700, 841]
    assert [-(-gx * gy // 128) for gx, gy in cc.SIZES] == [5, 6, 7]
    assert cc.FACTOR == 10.0 and cc.FLOOR == 1e-12
    assert len(cc.orderings(700)) == 6 and np.array_equal(cc.orderings(700)[0], np.arange(700))


def test_referee_on_a_matrix_with_a_known_factor():
    """The referee's own arithmetic: A = L L' with L of small integers is exact in fp64, so reference, LAPACK and the product
    residual are exact in the identity ordering, and kriging outputs equal their definition."""
    rng = np.random.default_rng(3)
    n = 40
    L = np.tril(rng.integers(-3, 4, size=(n, n))).astype(float)
    L[np.diag_indices(n)] = 2.0 ** rng.integers(0, 3, size=n)
    A = L @ L.T
    Y = rng.integers(-4, 5, size=(n, 3)).astype(float)
    B = L @ Y
    v = cc.referee_factor(A, B)
    assert abs(v.ref["logdet"] - np.sum(np.log(np.diag(L)))) < 1e-14
    assert np.array_equal(v.ref["Y"], Y)
    assert cc.product_residual(L, A) == 0.0
    assert cc.product_residual(L + 1e-3 * np.tril(np.ones((n, n))), A) > 1e-6
    vk = cc.referee_krige(A, B[:, 0], B[:, 1:].T)
    assert np.allclose(vk.ref["stochastic"], Y[:, 1:].T @ Y[:, 0], rtol=1e-15, atol=0)
    assert np.allclose(vk.ref["quadform"], np.sum(Y[:, 1:] ** 2, axis=0), rtol=1e-15, atol=0)
    assert cc.ratio(1.0 + 5e-12, 0.0, 1.0) == pytest.approx(5.0, rel=1e-3)
