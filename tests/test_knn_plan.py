"""The plan of the Vecchia neighbour search (cocons_amd/csrc/knn_plan.hpp) through the host-only diagnostic
entry cocons_debug_knn_plan, which computes the head, the levels, every level's grid, the clamped cells and the stopping
bound with the headers the kernels use.  No GPU.

The levels tile [head, n) with hi <= 2 lo; every grid covers its points within the cell caps; and FOR EVERY LEVEL, QUERY AND
TARGET among the level's points: with c >= 1 the Chebyshev distance between the target's cell and the query's clamped cell,
the brute-force d2 = fl(fl(dx dx) + fl(dy dy)) is >= bound(c - 1).  The ring walk stops after ring r when the m-th d2 is
below bound(r), and everything it has not seen then has c >= r + 1: the search is exact only if this holds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_reference as KR  # noqa: E402

CELLS_MAX = 1 << 20          # pattern_grid.hpp: PATTERN_CELLS_MAX, PATTERN_CELLS_AXIS_MAX


def _cases():
    rng = np.random.default_rng(11)
    g = np.arange(24.0)
    lat = np.array([(x, y) for y in g for x in g])
    return {
        "random": rng.uniform(0, 1, size=(700, 2)),
        "integer lattice": lat,
        "lattice / 39": lat / 39.0,
        "collinear (ny = 1)": np.column_stack([rng.permutation(300) * 0.01, np.full(300, 2.5)]),
        "two clusters 1e6 widths apart": np.vstack([rng.uniform(0, 1, size=(200, 2)),
                                                    1e6 + rng.uniform(0, 1, size=(200, 2))])[rng.permutation(400)],
        "box 1e6 times wider than high": rng.uniform(0, 1, size=(500, 2)) * np.array([1000.0, 0.001]),
        "all coincident": np.tile([[0.3, -0.4]], (150, 1)),
        "n = 1": np.array([[4.0, 5.0]]),
        "n = 2": np.array([[4.0, 5.0], [4.5, 5.25]]),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_levels_tile_grids_cover_and_the_bound_is_sound(name):
    locs = CASES[name]
    n = locs.shape[0]
    P = KR.plan(locs)
    head, levels = P["head"], P["levels"]
    assert head == min(n, 64)
    # the levels tile [head, n) with hi <= 2 lo
    at = head
    for lo, hi in levels:
        assert lo == at and lo < hi <= 2 * lo
        at = hi
    assert at == n and (levels or n <= head)
    if name == "random":
        assert len(levels) == 4                         # 64, 128, 256, 512 -> 700
    rng = np.random.default_rng(5)
    # grid l of the plan is over the first tops[l] points; the last one (all n points) is what plain kNN searches
    tops = [hi for _, hi in levels] + [n]
    assert P["geom"].shape[0] == len(tops)
    for level, top in enumerate(tops):
        pts = locs[:top]
        x0, y0, edge, nx, ny = P["geom"][level]
        nx, ny = int(nx), int(ny)
        assert edge > 0 and 1 <= nx <= CELLS_MAX and 1 <= ny <= CELLS_MAX and nx * ny <= CELLS_MAX
        assert x0 == pts[:, 0].min() and y0 == pts[:, 1].min()
        if name.startswith("collinear"):
            assert ny == 1
        span = float(np.max(pts.max(axis=0) - pts.min(axis=0)))
        q = KR.queries(pts, 0.05 * span if span > 0 else 0.1, rng)
        rmax = max(nx, ny) + 1
        R = KR.plan(locs, level, np.vstack([pts, q]), rmax)
        np.testing.assert_array_equal(R["geom"], P["geom"])
        tc, qc, bound = R["cells"][:top], R["cells"][top:], R["bounds"]
        # the level's points lie in [0, count), every clamped cell in [-1, count]
        assert tc[:, 0].min() >= 0 and tc[:, 0].max() < nx and tc[:, 1].min() >= 0 and tc[:, 1].max() < ny
        assert qc[:, 0].min() >= -1 and qc[:, 0].max() <= nx and qc[:, 1].min() >= -1 and qc[:, 1].max() <= ny
        assert bound[0] == 0.0 and np.all(np.diff(bound) >= 0)
        if rmax >= 1:
            assert 0.99 * edge * edge < bound[1] < edge * edge      # one cell, less the slack
        # every query (the level's own points, as in the self search, and the outside ones) against every target
        for Q, C in ((pts, tc), (q, qc)):
            dx = pts[None, :, 0] - Q[:, None, 0]
            dy = pts[None, :, 1] - Q[:, None, 1]
            d2 = dx * dx + dy * dy
            c = np.maximum(np.abs(tc[None, :, 0] - C[:, None, 0]), np.abs(tc[None, :, 1] - C[:, None, 1]))
            far = c >= 1
            assert np.all(d2[far] >= bound[c[far] - 1]), name
        if top > 8:
            assert far.any()


def test_refusals_leave_the_outputs_untouched():
    import ctypes
    from cocons_amd import _lib
    L = _lib.load()
    locs = np.array([0.0, 1.0, 2.0, 3.0, 0.0, 0.5, 0.0, 0.5])
    bad = locs.copy(); bad[5] = np.nan
    pts = np.zeros(6)
    head, geom = np.full(66, -7, dtype=np.int32), np.full(165, -7.0)
    cells, bounds = np.full(6, -7, dtype=np.int32), np.full(4, -7.0)
    ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.c_dp)

    def call(n=4, locs_=locs, level=0, m=3, pts_=pts, rmax=3, head_=head, geom_=geom, cells_=cells, bounds_=bounds):
        return L.cocons_debug_knn_plan(n, dp(locs_), level, m, dp(pts_), rmax, ip(head_), dp(geom_), ip(cells_), dp(bounds_))

    for kw in (dict(n=0), dict(locs_=None), dict(locs_=bad), dict(level=-1), dict(level=1), dict(m=-1), dict(pts_=None),
               dict(rmax=-2), dict(head_=None), dict(geom_=None), dict(cells_=None), dict(bounds_=None)):
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith("cocons_debug_knn_plan:"), kw
    assert np.all(head == -7) and np.all(geom == -7.0) and np.all(cells == -7) and np.all(bounds == -7.0)
    assert call() == 0 and head[0] == 4 and head[1] == 0
