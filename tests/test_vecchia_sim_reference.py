"""The reference of U^-1 on a Vecchia fit (tests/vecchia_sim_reference.py), without a GPU: the recursion equals a dense solve
with U, undoes the reference's whitening, is the Cholesky factor of Sigma when every predecessor is named, and its levels are
right on tables whose levels are known.  The problem is test_gpu_dense_sizes.problem's.

Bound: 1e-10 relative to the largest magnitude of the compared array.  Both sides are double computations on a triangular
system with cond(U) <= 64 on these cases and n <= 300, so they agree to about eps n cond(U) = 2.2e-16 * 300 * 64 = 4e-12."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_reference as VR  # noqa: E402
import vecchia_sim_reference as VS  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402

BOUND = 1e-10


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _table(n, m, holes=False):
    from cocons_amd import host
    nn = host.vecchia_neighbours(problem(n)[0], m).copy(order="F")
    if holes:
        nn[::3, m // 2] = 0
        nn[::3, 0] = 0
        nn[n // 2, :] = 0
    return nn


@pytest.mark.parametrize("n,m,holes", ((65, 10, False), (300, 30, False), (300, 30, True)))
def test_recursion_is_the_dense_solve_and_undoes_the_whitening(n, m, holes):
    S = problem(n)[6]
    nn = _table(n, m, holes)
    W = np.random.default_rng(n + m).standard_normal((n, 3))
    x = VS.unwhiten(S, nn, W)
    U = VR.precision_matrix(S, nn)[1]
    back = VR.whiten(S, nn, x)[0]
    errs = (_rel(x, np.linalg.solve(U, W)), _rel(back, W))
    print("vecchia-sim-report reference | solve(U, W), whiten(unwhiten(W)) n%d m%d%s | %.2e cond(U) %.1f"
          % (n, m, " holes" if holes else "", max(errs), np.linalg.cond(U)))
    assert max(errs) < BOUND, errs


def test_coefficients_are_the_rows_of_U():
    n, m = 65, 10
    S = problem(n)[6]
    nn = _table(n, m, True)
    U = VR.precision_matrix(S, nn)[1]
    coef = VS.coefficients(S, nn)
    for i in range(n):
        idx = VR.rows_of(nn, i)
        assert _rel(np.append(coef[i, :idx.size], coef[i, m]), U[i, np.append(idx, i)]) < BOUND
        assert np.all(coef[i, idx.size:m] == 0.0)


def test_all_predecessors_is_the_cholesky_factor():
    n = 64
    S = problem(65)[6][:n, :n]
    W = np.random.default_rng(64).standard_normal((n, 3))
    x = VS.unwhiten(S, VR.all_predecessors(n), W)
    err = _rel(x, np.linalg.cholesky(S) @ W)
    print("vecchia-sim-report reference | cholesky(S) @ W n64 m63 | %.2e" % err)
    assert err < BOUND


def test_fixed_rows_and_long_double():
    n, m, nf = 65, 10, 20
    S = problem(n)[6]
    nn = _table(n, m)
    rng = np.random.default_rng(5)
    xf, E = rng.standard_normal((nf, 2)), rng.standard_normal((n - nf, 2))
    x = VS.unwhiten(S, nn, E, n_fixed=nf, x_fixed=xf)
    assert np.array_equal(x[:nf], xf)
    # the whitening of the result gives E back in the rows that ran the recursion
    assert _rel(VR.whiten(S, nn, x)[0][nf:], E) < BOUND
    xl = VS.unwhiten(S, nn, E, n_fixed=nf, x_fixed=xf, long_double=True)
    err = _rel(x, np.asarray(xl, dtype=float))
    print("vecchia-sim-report reference | double against long double n65 m10 fixed 20 | %.2e" % err)
    assert err < 1e-12


def test_levels_of_known_tables():
    n = 641
    chain = np.zeros((n, 1), dtype=np.int32)
    chain[1:, 0] = np.arange(1, n)
    assert np.array_equal(VS.levels(chain), np.arange(1, n + 1))
    assert np.array_equal(VS.levels(chain, 64), np.concatenate([np.zeros(64), np.arange(1, n - 63)]))
    assert np.array_equal(VS.levels(np.zeros((n, 3), dtype=np.int32)), np.ones(n))
    holes = _table(65, 10, True)
    lv = VS.levels(holes)
    assert lv[0] == 1 and lv[32] == 1 and np.all(lv >= 1)       # row 33 (1-based) is the empty row
    for i in range(65):
        idx = VR.rows_of(holes, i)
        assert lv[i] == 1 + (lv[idx].max() if idx.size else 0)
    lf = VS.levels(holes, 64)
    assert np.all(lf[:64] == 0) and lf[64] == 1
