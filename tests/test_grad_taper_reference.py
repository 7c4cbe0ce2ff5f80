"""The numpy / scipy statement of the tapered gradient (tests/grad_taper_reference.py) against Richardson central differences
(steps h and h / 2) of the CPU oracle's GetNeg2loglikelihoodTaper with zero penalty, and the tile-envelope recursion against
numpy.linalg.inv -- all without a GPU.

Bound: 1e-8 of the gradient's largest component.  The differences carry the oracle's own rounding (cond(S) ~ 3e3, values
~ 1e3, step 1e-3: ~1e-10 of the gradient) and an O(h^4) truncation; the bound leaves them two digits."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_taper_reference as GT  # noqa: E402

from cocons_amd import host, workloads as wl  # noqa: E402
from oracle import oracle as O  # noqa: E402

N, DELTA = 250, 0.2


def _richardson(fun, x, h):
    g = np.zeros_like(x)
    for i in range(x.size):
        def d(step):
            xp, xm = x.copy(), x.copy()
            xp[i] += step
            xm[i] -= step
            return (fun(xp) - fun(xm)) / (2 * step)
        g[i] = (4 * d(h / 2) - d(h)) / 3
    return g


def _problem(r, seed):
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(N, 2))
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = 0.3 * np.array([1.0, -0.5, 0.25])
    z = rng.standard_normal((N, r))
    return locs, X, th, z, GT.wendland1_pattern(locs, DELTA)


def _par_pos(th, fixed=()):
    """every aspect free in every column, except the aspects in `fixed`, which keep th's first entry (a scalar par.pos)"""
    pp = OrderedDict()
    for k in host.ASPECTS:
        pp[k] = float(th[k][0]) if k in fixed else [True] * 3
    return pp


CASES = [
    ("free smoothness, r = 1", 1, None, True),
    ("free smoothness, r = 2", 2, None, True),
    ("nu = 0.5", 1, 0.5, True),
    ("nu = 1.5", 2, 1.5, True),
    ("nu = 2.5", 1, 2.5, True),
    ("nugget -Inf, r = 2", 2, None, False),
]


@pytest.mark.parametrize("name,r,nu,nugget", CASES, ids=[c[0] for c in CASES])
def test_reference_gradient_matches_oracle_differences(name, r, nu, nugget):
    locs, X, th, z, ref_taper = _problem(r, 31 + r)
    fixed = []
    sl = wl.SMOOTH_LIMITS
    if nu is not None:
        th["smooth"] = np.zeros(3)
        fixed.append("smooth")
        sl = (nu, nu)
    if not nugget:
        th["nugget"] = np.array([-np.inf, 0.0, 0.0])
        fixed.append("nugget")
    pp = _par_pos(th, fixed)
    x0 = wl.theta_vector_from_lists(th, pp)
    lam = (0.0, 0.0, 0.0)

    def fun(x):
        return O.GetNeg2loglikelihoodTaper(x, pp, ref_taper, locs, X, sl, z, N, lam, safe=False)

    tl = host.getModelLists(x0, pp, "diff")
    T = host.theta_table(tl)
    f, parts, gl, gq, gm = GT.neg2loglik_taper_grad(T, tl["mean"], locs, X, z, sl, ref_taper)
    assert abs(f - fun(x0)) <= 1e-11 * abs(f)
    assert abs(f - (r * (N * np.log(2 * np.pi) + 2 * parts[0]) + parts[1:].sum())) <= 1e-12 * abs(f)
    gt = gl + gq
    assert np.all(gt[2] == 0) and np.all(gt[3] == 0)          # aniso, tilt: not in the taper model
    if nu is not None:
        assert np.all(gt[4] == 0)
    g = OrderedDict(mean=gm)
    for t, k in enumerate(host.COV_ASPECTS):
        g[k] = gt[t]
    ana = host.getModelLists_grad(g, pp)
    num = _richardson(fun, x0, 1e-3)
    scale = np.max(np.abs(num))
    err = np.max(np.abs(ana - num))
    print("%s: max |analytic - Richardson| = %.3e of %.3e (%.2e relative)" % (name, err, scale, err / scale))
    assert err <= 1e-8 * scale, (name, err, scale)


def test_scaling_identity_of_the_reference():
    """S -> c S under (theta_sd0, theta_ng0) -> + log c (T is fixed): df/dsd0 + df/dng0 = r n - sum of the quadratic forms."""
    locs, X, th, z, ref_taper = _problem(2, 77)
    T = host.theta_table(th)
    f, parts, gl, gq, gm = GT.neg2loglik_taper_grad(T, th["mean"], locs, X, z, wl.SMOOTH_LIMITS, ref_taper)
    gt = gl + gq
    want = 2 * N - parts[1:].sum()
    assert abs(gt[0, 0] + gt[5, 0] - want) <= 1e-11 * 2 * N
    assert abs(gl[0, 0] + gl[5, 0] - 2 * N) <= 1e-11 * 2 * N


@pytest.mark.parametrize("tile", [16, 32])
def test_tile_envelope_recursion_reproduces_the_inverse(tile):
    """The selected inverse on the tile envelope of a banded (reverse Cuthill-McKee ordered) tapered matrix equals
    numpy.linalg.inv on every envelope tile; the pattern lies inside the envelope."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    n = 256
    rng = np.random.default_rng(5)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full(scale0=np.log(0.2))
    ci, rp, te = GT.wendland1_pattern(locs, 0.2)
    S, q = GT.taper_matrix(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, (ci, rp, te))
    perm = reverse_cuthill_mckee(csr_matrix((np.ones(ci.size), ci - 1, rp - 1), shape=(n, n)), symmetric_mode=True)
    S = S[np.ix_(perm, perm)]
    rows, cols = np.nonzero(S)
    hi = GT.tile_envelope(rows, cols, n, tile)
    assert np.all(np.diff(hi) >= 0) and hi[-1] == n // tile and hi[0] < n // tile      # monotone, and a real band
    Z = GT.selinv_envelope(S, tile, hi)
    ref = np.linalg.inv(S)
    inside = ~np.isnan(Z)
    assert np.all(inside[rows[rows >= cols], cols[rows >= cols]])                       # the pattern is inside the envelope
    err = np.max(np.abs(Z[inside] - ref[inside]))
    print("tile %d: max |Z - inv(S)| on the envelope = %.3e (entries up to %.3g)" % (tile, err, np.max(np.abs(ref))))
    assert err <= 1e-10 * np.max(np.abs(ref))


def test_recursion_needs_symmetric_diagonal_tiles():
    """A 60 x 60 grid, one grid row per tile (60 tile columns, band of 7 tiles, cond(S) ~ 1.4e3): with symmetrised diagonal tiles
    the sweep keeps 1e-10 of max |S^-1| down to the first tile column; without, the antisymmetric rounding error of the
    diagonal tiles grows along the sweep (observed: 1.3e-8 against 5e-14 absolute) -- the witness for what the kernel does."""
    g = 60
    n = g * g
    locs = wl.grid_locs(g)
    X = wl.design_from_locs(locs)["std.covs"]
    sp = 1.0 / (g - 1)
    th = wl.theta_full(scale0=np.log(16 * sp))
    S, q = GT.taper_matrix(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, GT.wendland1_pattern(locs, 6.2 * sp))
    rows, cols = np.nonzero(S)
    hi = GT.tile_envelope(rows, cols, n, g)
    ref = np.linalg.inv(S)
    err = {}
    for sym in (True, False):
        Z = GT.selinv_envelope(S, g, hi, symmetric=sym)
        inside = ~np.isnan(Z)
        err[sym] = np.max(np.abs(Z[inside] - ref[inside]))
    print("symmetrised %.3e, plain %.3e (entries up to %.3g)" % (err[True], err[False], np.max(np.abs(ref))))
    assert err[True] <= 1e-10 * np.max(np.abs(ref))
    assert err[False] > 100 * err[True]
