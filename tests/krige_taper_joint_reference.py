"""The ring solve of cocons_krige_taper_joint in numpy, with a small tile edge: tests/krige_taper_reference.py's loop with a
ring of Wr = min(W + D - 1, nt) slots (tile column I in slot I mod Wr; the live window and the loads stay those of W), and
S -= V_g V_g' behind the diag step of the last tile column of every group of D consecutive tile columns (and of the last,
possibly partial, group).  The device code (solve.hip, launch_krige_band_solve with S set) takes exactly these steps.

The ring is instrumented: every slot remembers which tile column it holds and whether that column's group product has read
it.  A load that meets a solved tile column whose product has not been taken raises."""
import numpy as np

from krige_taper_reference import load_schedule  # noqa: F401  (what the loads are compared with)


class SlotOverwritten(AssertionError):
    pass


def ring_schur(L, hi, T, W, D, rows_ci, rows_val, S_uu, slots=None):
    """S_uu - sum_g V_g V_g' for the rows given as (sorted 0-based columns, values); also returns the (step, tile) loads,
    the number of ring columns allocated and the groups [(first tile column, one past the last)] whose product was taken.
    slots: another number of ring slots than min(W + D - 1, nt) (the tests show that one fewer is caught)."""
    nt, M = L.shape[0] // T, len(rows_ci)
    Wr = min(W + D - 1, nt) if slots is None else slots
    ring = np.zeros((M, Wr * T))
    holds = [None] * Wr               # tile column in the slot
    consumed = [True] * Wr            # ... and whether its group's product has read it (an empty slot: nothing to lose)
    S = np.array(S_uu, dtype=float)
    loads, groups = [], []
    buckets = [[] for _ in range(nt)]
    for i in range(M):
        for c, v in zip(rows_ci[i], rows_val[i]):
            buckets[c // T].append((i, c % T, v))

    def load(J, I):
        k = I % Wr
        if not consumed[k]:
            raise SlotOverwritten("step %d: the load of tile %d meets tile %d, whose product was not taken" % (J, I, holds[k]))
        s = k * T
        ring[:, s:s + T] = 0.0
        for i, c, v in buckets[I]:
            ring[i, s + c] = v
        holds[k], consumed[k] = I, False
        loads.append((J, I))

    for I in range(min(W, nt)):
        load(0, I)
    for J in range(nt):
        if J > 0 and J + W - 1 < nt:
            load(J, J + W - 1)
        k = J % Wr
        assert holds[k] == J
        s = k * T
        V = np.linalg.solve(L[J * T:(J + 1) * T, J * T:(J + 1) * T], ring[:, s:s + T].T).T       # diag
        ring[:, s:s + T] = V
        if (J + 1) % D == 0 or J + 1 == nt:                                                         # the group's product
            g0 = J // D * D
            for t in range(g0, J + 1):
                kt = t % Wr
                assert holds[kt] == t and not consumed[kt]
                Vt = ring[:, kt * T:(kt + 1) * T]
                S -= Vt @ Vt.T
                consumed[kt] = True
            groups.append((g0, J + 1))
        for I in range(J + 1, hi[J]):                                                               # update
            ki = I % Wr
            assert holds[ki] == I
            ring[:, ki * T:(ki + 1) * T] -= V @ L[I * T:(I + 1) * T, J * T:(J + 1) * T].T
    assert all(consumed)
    return S, loads, ring.shape[1], groups
