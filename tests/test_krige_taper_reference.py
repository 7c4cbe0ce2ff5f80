"""The ring loop of the tapered kriging (tests/krige_taper_reference.py) against a dense solve, on the CPU: envelopes with
W < nt (irregular and monotone, the ring wrapping several times), W = nt and nt = 1; an empty row, a row whose only
entries lie in the last tile and a row that spans two tiles; and the load rule stated explicitly."""
import numpy as np
import pytest

from krige_taper_reference import envelope, load_schedule, ring_solve

T = 4


def _banded_spd(n, bw, rng):
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(max(0, i - int(bw[i])), i):
            A[i, j] = A[j, i] = 0.3 * rng.standard_normal()
    return A + np.eye(n) * (np.abs(A).sum(1).max() + 1.0)


def _case(name):
    rng = np.random.default_rng(11)
    if name == "irregular":                  # W = 3 of 13 tile columns: the ring wraps four times
        nt = 13
        bw = rng.integers(2, 9, size=T * nt)
    elif name == "narrow":                   # W = 2 of 16: every slot reused seven times
        nt = 16
        bw = np.full(T * nt, 3)
    elif name == "full":                     # W = nt: the ring is the whole right-hand side
        nt = 5
        bw = np.full(T * nt, T * nt)
    else:                                    # one tile
        nt = 1
        bw = np.full(T, T)
    n = T * nt
    A = _banded_spd(n, bw, rng)
    L = np.linalg.cholesky(A)
    hi, W = envelope(L, T)
    return rng, n, nt, A, L, hi, W


def _rows(rng, n, nt):
    """rows of the chunk: random short rows, an empty row (3), only the last tile (4), across the first tile edge (5)"""
    ci, val = [], []
    for i in range(9):
        if i == 3:
            c = np.array([], dtype=int)
        elif i == 4:
            c = np.arange(n - T, n)[::2]
        elif i == 5 and nt > 1:
            c = np.array([T - 2, T - 1, T, T + 1])
        else:
            k = int(rng.integers(1, min(8, n) + 1))
            c0 = int(rng.integers(0, n - k + 1))
            c = np.sort(rng.choice(np.arange(c0, min(n, c0 + 12)), size=k, replace=False))
        ci.append(list(c))
        val.append(list(rng.standard_normal(len(c))))
    return ci, val


@pytest.mark.parametrize("name", ["irregular", "narrow", "full", "single"])
def test_ring_solve_matches_a_dense_solve(name):
    rng, n, nt, A, L, hi, W = _case(name)
    if name in ("irregular", "narrow"):
        assert W < nt and nt // W >= 4
    if name == "full":
        assert W == nt
    ci, val = _rows(rng, n, nt)
    C = np.zeros((len(ci), n))
    for i, (c, v) in enumerate(zip(ci, val)):
        C[i, c] = v
    r = rng.standard_normal(n)
    w = np.linalg.solve(L, r)
    st, qd, loads, width = ring_solve(L, hi, T, W, ci, val, w)
    X = np.linalg.solve(A, C.T)
    st_ref, qd_ref = r @ X, np.sum(C * X.T, axis=1)
    # both sides are backward stable solves of a matrix with condition < 10: 64 eps of the largest value is ample
    assert np.max(np.abs(st - st_ref)) <= 64 * np.finfo(float).eps * np.max(np.abs(st_ref))
    assert np.max(np.abs(qd - qd_ref)) <= 64 * np.finfo(float).eps * np.max(np.abs(qd_ref))
    assert st[3] == 0.0 and qd[3] == 0.0                     # the empty row: exactly zero
    assert width == W * T                                    # never rows x n when W < nt
    assert loads == load_schedule(nt, W)
    assert sorted(I for _, I in loads) == list(range(nt))    # every tile column enters the ring exactly once


def test_load_rule():
    """Which tile enters at which step: the first min(W, nt) at step 0, then tile J + W - 1 at step J -- the slot
    (J + W - 1) mod W = (J - 1) mod W is the one tile J - 1 has just left -- and no tile after nt - 1."""
    assert load_schedule(5, 2) == [(0, 0), (0, 1), (1, 2), (2, 3), (3, 4)]
    assert load_schedule(3, 3) == [(0, 0), (0, 1), (0, 2)]
    assert load_schedule(2, 5) == [(0, 0), (0, 1)]
    assert load_schedule(1, 1) == [(0, 0)]
    for nt, W in ((13, 3), (16, 2), (7, 7), (9, 4)):
        for J, I in load_schedule(nt, W):
            if J > 0:
                assert I == J + W - 1 and I % W == (J - 1) % W
            # a tile is in the ring before the first step that may update it: I < hi[K] <= K + W needs K >= I - W + 1
            assert J <= max(I - W + 1, 0)


def test_a_tile_is_never_updated_before_it_is_loaded_nor_after_it_left():
    rng, n, nt, A, L, hi, W = _case("irregular")
    loaded_at = dict((I, J) for J, I in load_schedule(nt, W))
    for J in range(nt):
        for I in range(J + 1, hi[J]):
            assert loaded_at[I] <= J and I <= J + W - 1
