"""What the tests of the Vecchia neighbour search share: the numpy brute force of the rule -- the m candidates
with the smallest key (d2, index), d2 = fl(fl(dx dx) + fl(dy dy)), no square root, ties to the lower index, rows nearest
first and zero-padded --, the point sets, the queries of test_pattern_grid.py, and the plan through cocons_debug_knn_plan."""
import ctypes

import numpy as np

SEED = 20261020
LEVELS_MAX = 32


def _d2(q, c):
    dx = c[None, :, 0] - q[:, None, 0]
    dy = c[None, :, 1] - q[:, None, 1]
    return dx * dx + dy * dy


def brute_self(locs, m, chunk=512):
    """row i: the m nearest among rows 0 .. i - 1 (1-based, 0 = none)"""
    locs = np.ascontiguousarray(locs, dtype=np.float64)
    n = locs.shape[0]
    nn = np.zeros((n, m), dtype=np.int32, order="F")
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        if r1 <= 1:
            continue
        D = _d2(locs[r0:r1], locs[:r1 - 1])
        D[np.arange(r1 - 1)[None, :] >= np.arange(r0, r1)[:, None]] = np.inf
        order = np.argsort(D, axis=1, kind="stable")[:, :m]          # stable: ties to the lower index
        keep = np.isfinite(np.take_along_axis(D, order, axis=1))
        nn[r0:r1, :order.shape[1]] = np.where(keep, order + 1, 0)
    return nn


def brute_pred(locs, q, m, chunk=512):
    """row i: the m nearest of locs to q[i] (1-based, 0 = none)"""
    locs = np.ascontiguousarray(locs, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    nn = np.zeros((q.shape[0], m), dtype=np.int32, order="F")
    for r0 in range(0, q.shape[0], chunk):
        order = np.argsort(_d2(q[r0:r0 + chunk], locs), axis=1, kind="stable")[:, :m]
        nn[r0:r0 + chunk, :order.shape[1]] = order + 1
    return nn


def uniform(n):
    return np.random.default_rng(SEED).uniform(0, 1, size=(n, 2))


def lattice(nx, ny):
    return np.array([(float(x), float(y)) for y in range(ny) for x in range(nx)])


def special_sets():
    rng = np.random.default_rng(SEED + 1)
    lat = lattice(24, 24)
    return {
        "lattice": lat,
        "lattice permuted": lat[rng.permutation(lat.shape[0])],
        "lattice / 39": lat / 39.0,
        "all coincident": np.tile([[0.3, -0.4]], (150, 1)),
        "collinear": np.column_stack([rng.permutation(300) * 0.01, np.full(300, 2.5)]),
        "two clusters": np.vstack([rng.uniform(0, 1, size=(200, 2)), 1e6 + rng.uniform(0, 1, size=(200, 2))])[
            rng.permutation(400)],
    }


def queries(locs, delta, rng):
    """test_pattern_grid.py's _queries: inside, on the edge of, and outside the targets' box (near and far beyond)"""
    lo, hi = locs.min(axis=0), locs.max(axis=0)
    span = np.maximum(hi - lo, delta)
    inside = lo + rng.uniform(0, 1, size=(40, 2)) * (hi - lo)
    edge = np.array([[lo[0], lo[1]], [hi[0], hi[1]], [lo[0], hi[1]], [hi[0], lo[1]], [lo[0], 0.5 * (lo[1] + hi[1])],
                     [0.5 * (lo[0] + hi[0]), hi[1]]])
    near = np.array([[lo[0] - 0.5 * delta, lo[1]], [hi[0] + 0.99 * delta, hi[1]], [lo[0], lo[1] - delta],
                     [hi[0] + 0.7 * delta, hi[1] + 0.7 * delta], [lo[0] - 0.7 * delta, hi[1] + 0.7 * delta]])
    far = np.array([[lo[0] - 3 * span[0], lo[1]], [hi[0] + 1e3 * span[0], hi[1] + 1e3 * span[1]], [lo[0], hi[1] + 2.5 * delta],
                    [hi[0] + 1e12 * span[0], lo[1] - 1e12 * span[1]]])
    return np.vstack([inside, edge, near, far, locs[:30], locs[:10] + 0.5 * delta])


def plan(locs, level=0, pts=None, rmax=-1):
    """{"head", "levels": [(lo, hi)], "geom": (L + 1) x 5, "cells": the clamped cells of pts on grid `level`, "bounds"}"""
    from cocons_amd import _lib
    L = _lib.load()
    locs = np.asfortranarray(locs, dtype=np.float64)
    pts = np.zeros((0, 2), order="F") if pts is None else np.asfortranarray(pts, dtype=np.float64)
    n, m = locs.shape[0], pts.shape[0]
    head = np.zeros(2 + 2 * LEVELS_MAX, dtype=np.int32)
    geom = np.zeros((LEVELS_MAX + 1, 5))
    cells = np.zeros((max(m, 1), 2), dtype=np.int32)
    bounds = np.zeros(max(rmax + 1, 1))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    rc = L.cocons_debug_knn_plan(n, dp(locs), int(level), m, dp(pts), int(rmax), ip(head), dp(geom), ip(cells), dp(bounds))
    assert rc == 0, _lib.last_error()
    nl = int(head[1])
    return {"head": int(head[0]), "levels": [(int(head[2 + 2 * l]), int(head[3 + 2 * l])) for l in range(nl)],
            "geom": geom[:nl + 1].copy(), "cells": cells[:m].copy(), "bounds": bounds[:rmax + 1].copy()}
