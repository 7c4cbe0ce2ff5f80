"""The uniform grid of the taper-pattern builder (cocons_amd/csrc/pattern_grid.hpp) through the host-only diagnostic entry
cocons_debug_pattern_cells, which computes the geometry and the clamped cells with the header the kernels use.  No GPU.

For every point set and delta: the cell edge is >= delta, every clamped cell coordinate lies in [-1, count], the targets'
own cells lie in [0, count), and every pair (query, target) with d <= delta -- numpy brute force, d = sqrt(dx dx + dy dy) --
has the target's cell inside the 3 x 3 block around the query's clamped cell, which is what the kernels scan."""
import ctypes

import numpy as np
import pytest

CELLS_MAX = 1 << 20          # pattern_grid.hpp: PATTERN_CELLS_MAX


def _cells(locs, delta, pts):
    from cocons_amd import _lib
    L = _lib.load()
    locs = np.asfortranarray(locs, dtype=np.float64)
    pts = np.asfortranarray(pts, dtype=np.float64)
    n, m = locs.shape[0], pts.shape[0]
    geom = np.zeros(5)
    cells = np.zeros((m, 2), dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    rc = L.cocons_debug_pattern_cells(n, dp(locs), float(delta), m, dp(pts), dp(geom),
                                      cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == 0, _lib.last_error()
    return geom, cells


def _queries(locs, delta, rng):
    """inside, on the edge of, and outside the targets' box (within delta of it and far beyond)"""
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


def _cases():
    rng = np.random.default_rng(11)
    g = np.arange(40) / 39.0
    lattice = np.array([(x, y) for y in g for x in g])
    return {
        "random": (rng.uniform(0, 1, size=(600, 2)), 0.07),
        "lattice, delta = the spacing": (lattice, 1.0 / 39.0),
        "collinear (zero-height box)": (np.column_stack([np.arange(300) * 0.01, np.full(300, 2.5)]), 0.035),
        "collinear along y": (np.column_stack([np.full(300, -1.0), np.arange(300) * 0.01]), 0.035),
        "all coincident (zero-extent box)": (np.tile([[0.3, -0.4]], (50, 1)), 0.1),
        "one target": (np.array([[4.0, 5.0]]), 0.25),
        "offset by 1e6": (1e6 + rng.uniform(0, 1, size=(500, 2)), 0.05),
        "negative coordinates": (-5.0 + rng.uniform(-1, 1, size=(500, 2)), 0.11),
        "delta larger than the domain": (rng.uniform(0, 1, size=(300, 2)), 3.0),
        "delta so small that the cap enlarges the edge": (rng.uniform(0, 1, size=(400, 2)), 1e-5),
        "tiny delta, collinear": (np.column_stack([np.arange(200) * 1.0, np.zeros(200)]), 1e-9),
        "anisotropic box": (rng.uniform(0, 1, size=(400, 2)) * np.array([1000.0, 0.01]), 0.02),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_neighbours_lie_in_the_three_by_three_block(name):
    locs, delta = CASES[name]
    rng = np.random.default_rng(5)
    pts = _queries(locs, delta, rng)
    geom, qc = _cells(locs, delta, pts)
    _, tc = _cells(locs, delta, locs)
    x0, y0, edge, nx, ny = geom[0], geom[1], geom[2], int(geom[3]), int(geom[4])
    assert edge >= delta and nx >= 1 and ny >= 1 and nx * ny <= CELLS_MAX
    assert x0 == locs[:, 0].min() and y0 == locs[:, 1].min()
    if name.startswith(("delta so small", "tiny delta")):
        assert edge > 2 * delta                      # the cap, not delta, sets the edge
    else:
        assert edge <= delta * (1 + 1e-5)
    # clamped cells lie in [-1, count], the targets' own in [0, count)
    assert qc[:, 0].min() >= -1 and qc[:, 0].max() <= nx and qc[:, 1].min() >= -1 and qc[:, 1].max() <= ny
    assert tc[:, 0].min() >= 0 and tc[:, 0].max() < nx and tc[:, 1].min() >= 0 and tc[:, 1].max() < ny
    # brute force: all pairs
    dx = pts[:, None, 0] - locs[None, :, 0]
    dy = pts[:, None, 1] - locs[None, :, 1]
    d = np.sqrt(dx * dx + dy * dy)
    qi, ti = np.nonzero(d <= delta)
    assert qi.size > 0
    assert np.all(np.abs(qc[qi, 0] - tc[ti, 0]) <= 1) and np.all(np.abs(qc[qi, 1] - tc[ti, 1]) <= 1)
    # the far queries are clamped to one outside the range
    assert set(qc[:, 0]) & {-1, nx} and set(qc[:, 1]) & {-1, ny}


def test_pairs_at_exactly_delta_along_an_axis_stay_adjacent():
    """Targets on a lattice whose spacing is exactly delta, queries on the lattice points: cell coordinates of points exactly
    delta apart differ by at most one although the quotients are rounded."""
    for delta in (0.1, 1.0 / 3.0, 0.7, 1e-3):
        k = np.arange(400)
        locs = np.column_stack([k * delta, (k % 7) * delta])
        _, c = _cells(locs, delta, locs)
        order = np.argsort(locs[:, 0], kind="stable")
        assert np.all(np.abs(np.diff(c[order, 0])) <= 1)
        dx = locs[:, None, 0] - locs[None, :, 0]
        dy = locs[:, None, 1] - locs[None, :, 1]
        qi, ti = np.nonzero(np.sqrt(dx * dx + dy * dy) <= delta)
        assert np.all(np.abs(c[qi] - c[ti]) <= 1)
