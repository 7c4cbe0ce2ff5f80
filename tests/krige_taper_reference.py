"""The ring solve of cocons_krige_taper_apply in numpy, with a small tile edge: V = C L^-T for a sparse chunk C and a
lower factor L that fills only the tile envelope J <= I < hi[J], right-looking over the tile columns with the running
right-hand side held in a ring of W = max_J (hi[J] - J) tile columns (tile column I in slot I mod W).  The device code
(solve.hip, launch_krige_band_solve) takes exactly these steps per tile column J: load, diag, update."""
import numpy as np


def envelope(L, T):
    """(hi, W) of a lower factor: hi[J] = one past the last tile row of tile column J that holds a non-zero, made
    monotone (the handle's envelope is), and W = max_J (hi[J] - J)."""
    n = L.shape[0]
    nt = n // T
    hi = [J + 1 for J in range(nt)]
    for j in range(n):
        last = np.nonzero(L[:, j])[0].max()
        hi[j // T] = max(hi[j // T], last // T + 1)
    for J in range(1, nt):
        hi[J] = max(hi[J], hi[J - 1])
    return hi, max(hi[J] - J for J in range(nt))


def load_schedule(nt, W):
    """[(step J, tile loaded)]: at J = 0 the tiles 0 .. min(W, nt) - 1, at J > 0 the tile J + W - 1 if it exists --
    into the slot tile J - 1 just left."""
    out = [(0, I) for I in range(min(W, nt))]
    out += [(J, J + W - 1) for J in range(1, nt) if J + W - 1 < nt]
    return out


def ring_solve(L, hi, T, W, rows_ci, rows_val, w):
    """stochastic[i] = V(i, :) w and quadform[i] = V(i, :) V(i, :)' for the rows given as (sorted 0-based columns, values);
    also returns the (step, tile) loads that were made and the largest number of ring columns ever allocated."""
    nt, M = L.shape[0] // T, len(rows_ci)
    ring = np.zeros((M, W * T))
    st, qd = np.zeros(M), np.zeros(M)
    loads = []
    # the host's buckets: every stored entry goes to the bucket of its tile column once
    buckets = [[] for _ in range(nt)]
    for i in range(M):
        for c, v in zip(rows_ci[i], rows_val[i]):
            buckets[c // T].append((i, c % T, v))

    def load(J, I):
        s = (I % W) * T
        ring[:, s:s + T] = 0.0
        for i, c, v in buckets[I]:
            ring[i, s + c] = v
        loads.append((J, I))

    for I in range(min(W, nt)):
        load(0, I)
    for J in range(nt):
        if J > 0 and J + W - 1 < nt:
            load(J, J + W - 1)
        s = (J % W) * T
        V = np.linalg.solve(L[J * T:(J + 1) * T, J * T:(J + 1) * T], ring[:, s:s + T].T).T       # diag
        ring[:, s:s + T] = V
        st += V @ w[J * T:(J + 1) * T]
        qd += np.sum(V * V, axis=1)
        for I in range(J + 1, hi[J]):                                                               # update
            si = (I % W) * T
            ring[:, si:si + T] -= V @ L[I * T:(I + 1) * T, J * T:(J + 1) * T].T
    return st, qd, loads, ring.shape[1]
