"""Taper problems at the sizes where the tile arithmetic of a tapered fit degenerates (test infrastructure; numpy only, nothing
of the library is imported or read): one observation, one tile column full or nearly empty, sizes that are whole tiles, the
odd tile counts, and the first size whose band buffer packs.  The rules (pattern, envelope, order) are those of tests/
taper_envelope_cases.py, imported; tests/test_taper_size_cases.py holds the table below on the CPU, tests/
test_gpu_taper_sizes.py holds the library against it.

problem(n) -> taper_envelope_cases.Problem from fixed seeds: uniform sites on the unit square; the design is the intercept
alone for n < 3 (the standardised [1, x, y] is undefined at n = 1 and rank-deficient at n = 2) and [1, N(0, 0.5^2),
N(0, 0.5^2)] otherwise; theta_full() cut to the design's columns; two realisations; Wendland-1 taper of range 0.25 up to
n = 384 and 0.15 above; 130 prediction rows (two 64-row chunks and a chunk of 2) of which row ON_TOP lies on an observation
and row EMPTY at (4, 4) has no neighbour, and the Wendland-1 pattern among the prediction rows (uu_pattern).

The row on top of an observation: the model gives a coincident pair the prediction site's whole variance, nugget included, as
their covariance, whatever the two designs say about the site.  For the marginal prediction that is a number like any other:
with p = 3 and unrelated designs the predictive variance there comes out positive at some sizes and negative at others (the
prediction reports its absolute value), and it is nowhere near zero (tests/test_taper_size_cases.py).  With the intercept
alone (n < 3) the two designs are equal and the predictive variance of that row IS zero: the prediction reproduces the
observation, and sd.pred there is the square root of rounding error.  The JOINT predictive covariance of a set that holds
this row is singular when the designs are equal and in general indefinite when they are not (smallest eigenvalue down to -0.99
over these sizes; +0.012 at least without the row): its entries are compared on all 130 rows, draws are asked for on the
other 129 (draw_rows).

In the library's own order (reverse Cuthill-McKee):

    n              nt  W  packed  envelope
    1 ... 128       1  1  no      hi = [1]
    129, 192, 256   2  2  no      hi = [2, 2]
    257, 384        3  3  no      hi = [3, 3, 3]
    512             4  4  no      hi = [4, 4, 4, 4], the floor alone
    640             5  4  yes     hi = [4, 4, 5, 5, 5], the floor alone: the first packed size, no ragged tile

In the caller's order (sites as drawn) the floor decides up to nt = 4 as well; at n = 640 every tile column reaches the last
tile row (W = nt = 5, unpacked).
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np

import taper_envelope_cases as TE
from taper_envelope_cases import (Problem, envelope_of, pattern, pred_pattern, rcm_order, take_rows,  # noqa: F401
                                  theta_full)

TILE = TE.TILE
TAPER_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 192, 256, 257, 384, 512, 640)
CALLER_ORDER_SIZES = (128, 640)            # also run with the observations in the caller's order
M_PRED = 130
ON_TOP, EMPTY = 70, 128                    # the second 64-row chunk; the chunk of two rows
R = 2

# n -> (nt, W, packed, hi) in the library's order
TABLE = {n: (1, 1, False, [1]) for n in TAPER_SIZES if n <= 128}
TABLE.update({n: (2, 2, False, [2, 2]) for n in (129, 192, 256)})
TABLE.update({n: (3, 3, False, [3, 3, 3]) for n in (257, 384)})
TABLE[512] = (4, 4, False, [4, 4, 4, 4])
TABLE[640] = (5, 4, True, [4, 4, 5, 5, 5])


def delta_of(n):
    return 0.25 if n <= 384 else 0.15


def columns_of(n):
    """p: the intercept alone below three observations"""
    return 1 if n < 3 else 3


def _design(rng, rows, p):
    return np.asfortranarray(np.column_stack([np.ones(rows)] + [rng.standard_normal(rows) * 0.5 for _ in range(p - 1)]))


@functools.lru_cache(maxsize=None)
def problem(n, rcm=True):
    """The case of n observations, from fixed seeds; computed once, every array read-only.  rcm = False: the same problem for
    a handle that keeps the caller's order.  special = (None, EMPTY, ON_TOP): there is no row picked for its many neighbours."""
    if not rcm:
        return problem(n)._replace(name="n%d_caller" % n, rcm=False)
    rng = np.random.default_rng(12800 + n)
    p = columns_of(n)
    delta = delta_of(n)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = _design(rng, n, p)
    theta = OrderedDict((k, v[:p].copy()) for k, v in theta_full().items())
    z = np.asfortranarray(rng.standard_normal((n, R)))
    lp = rng.uniform(0, 1, size=(M_PRED, 2))
    lp[ON_TOP] = locs[(3 * n) // 7]
    lp[EMPTY] = np.array([4.0, 4.0])
    Xp = _design(rng, M_PRED, p)
    ref_taper = pattern(locs, delta)
    pred_taper = pred_pattern(lp, locs, delta)
    out = Problem("n%d" % n, n, delta, True, locs, X, theta, z, ref_taper, lp, Xp, pred_taper, (None, EMPTY, ON_TOP),
                  "n%d" % n, np.arange(n))
    for a in (locs, X, z, lp, Xp, out.perm) + ref_taper + pred_taper + tuple(theta.values()):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def uu_pattern(n):
    """the Wendland-1 pattern among the prediction rows of problem(n) (row EMPTY holds its diagonal alone)"""
    p = problem(n)
    out = pattern(p.lp, p.delta)
    for a in out:
        a.setflags(write=False)
    return out


def sub_pattern(uu, idx):
    """the pattern of the prediction rows idx (ascending) among themselves, renumbered"""
    ci, rp, ent = uu
    m = len(rp) - 1
    idx = np.asarray(idx)
    assert np.all(np.diff(idx) > 0)
    new = np.full(m, -1)
    new[idx] = np.arange(idx.size)
    rows = np.repeat(np.arange(m), np.diff(rp))
    keep = (new[rows] >= 0) & (new[ci - 1] >= 0)
    rp2 = np.concatenate([[1], 1 + np.cumsum(np.bincount(new[rows[keep]], minlength=idx.size))])
    return (new[ci[keep] - 1] + 1).astype(np.int32), rp2.astype(np.int32), ent[keep]


def draw_rows():
    """the prediction rows a draw is asked for: all but the row on top of an observation (module docstring)"""
    return np.delete(np.arange(M_PRED), ON_TOP)


def shifted(th):
    """another theta on the same handle: the shift of taper_envelope_cases.shifted (scale and nugget intercepts), for a theta
    of any number of columns"""
    out = OrderedDict((k, np.array(v, dtype=float)) for k, v in th.items())
    out["scale"][0] += 0.15
    out["nugget"][0] += 0.2
    return out


def order_of(prob):
    """the order the handle will take the observations in, 1-based"""
    return TE.order_of(prob)


def assert_shape(n, nt, hi, W, packed, rcm=True):
    """The size's row of the table (module docstring) for an envelope as envelope_of returns it -- on the restated order on the
    CPU, on the order the handle reports on the GPU."""
    want_nt = (n + TILE - 1) // TILE
    assert nt == want_nt == len(hi) and hi[-1] == nt
    if rcm:
        assert (nt, W, packed, list(map(int, hi))) == TABLE[n], (n, nt, W, packed, hi)
    else:
        assert W == nt and not packed and all(int(h) == nt for h in hi), (n, nt, W, packed, hi)
    assert packed == (n == 640 and rcm)
