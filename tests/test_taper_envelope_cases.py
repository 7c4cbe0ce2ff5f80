"""tests/taper_envelope_cases.py (the cases and the restated envelope rule of tests/test_gpu_taper_envelopes.py) on the CPU:
every case shows the shape it claims, the restated envelope holds the whole dense Cholesky factor in the order it was made
for (and notices when it is one tile too tight), the inputs are conditioned like those the suite's tolerances were set at,
the prediction sets hold the rows they promise, and the ring's load rule covers the case's (nt, W); and the library's own
envelope rule and packed band layout (cocons_amd/csrc/band_plan.hpp, compiled into tests/band_plan_main.cpp by the host
compiler) agree with the restatement integer for integer, and so does its bucket sort of a chunk's entries by tile column
(band_buckets, what tapered kriging scatters a chunk into the ring by).  The cases wider than eight tile rows (TE.WIDE) must
also show that their far tiles matter: the factor with every tile (I, J), I - J >= 8, set to zero gives another quadratic
form and another kriging prediction, by a hundred times the suite's tolerances at least; and the tiles the two-column block
rule adds to a flat band are shown to be exactly zero, so nobody counts them as coverage.  No GPU."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_taper_reference as GT  # noqa: E402
import taper_envelope_cases as TE  # noqa: E402
from krige_taper_reference import load_schedule  # noqa: E402

COND_CAP = 1e5
COND_CAP_WIDE = 1e3               # the wide cases keep ROUTE_TOL by staying well conditioned
QUAD_MOVES = 100 * 1e-8           # 100 x N2LL_RTOL (tests/test_gpu_parity.py)
KRIGE_MOVES = 100 * 1e-10         # 100 x the stochastic bound of test_taper_predict_vs_oracle


@functools.lru_cache(maxsize=None)
def _matrix(name):
    from cocons_amd.host import theta_table
    p = TE.problem(name)
    if p.base != name and np.array_equal(p.perm, np.arange(p.n)) and np.array_equal(p.ref_taper[2], TE.problem(p.base).ref_taper[2]):
        return _matrix(p.base)                                  # the same observations and pattern in another handle order
    S, _ = GT.taper_matrix(theta_table(p.theta), p.locs, p.X, TE.SMOOTH_LIMITS, p.ref_taper)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _envelope(name):
    p = TE.problem(name)
    order = TE.order_of(p)
    return (order,) + TE.envelope_of(p.n, p.ref_taper[0], p.ref_taper[1], order)


@functools.lru_cache(maxsize=None)
def _factor(name):
    """the dense factor of S in the handle's order, padded by the identity to whole tiles"""
    p = TE.problem(name)
    o = _envelope(name)[0] - 1
    nt = (p.n + TE.TILE - 1) // TE.TILE
    Sp = np.eye(nt * TE.TILE)
    Sp[:p.n, :p.n] = _matrix(name)[np.ix_(o, o)]
    return np.linalg.cholesky(Sp)


def _tiles_outside(L, hi):
    """tiles (I, J), I >= hi[J], of the lower factor that hold a non-zero"""
    T = TE.TILE
    return [(I, J) for J in range(len(hi)) for I in range(int(hi[J]), len(hi)) if np.any(L[I * T:(I + 1) * T, J * T:(J + 1) * T])]


@pytest.mark.parametrize("name", TE.NAMES)
def test_shape_conditioning_and_containment(name):
    p = TE.problem(name)
    order, nt, hi, W, packed = _envelope(name)
    S = _matrix(name)
    cond = float(np.linalg.cond(S))
    print("%s: n %d nt %d W %d hi - c %s mirrored %s cond(S) %.3g"
          % (name, p.n, nt, W, (hi - np.arange(nt)).tolist(), (TE.mirrored_envelope(hi) - np.arange(nt)).tolist(), cond))
    TE.assert_shape(name, nt, hi, W, packed)
    if not p.rcm:
        assert np.array_equal(order, np.arange(1, p.n + 1))
    else:
        assert sorted(order.tolist()) == list(range(1, p.n + 1)) and not np.array_equal(order, np.arange(1, p.n + 1))
    assert cond <= (COND_CAP_WIDE if name in TE.WIDE else COND_CAP), cond
    assert np.allclose(S, S.T, rtol=1e-14, atol=0) and np.all(np.isfinite(S))      # (the two orders of a product: last bit)
    assert _tiles_outside(_factor(name), hi) == []
    # the mirrored envelope holds the flipped factor in the same way
    hib = TE.mirrored_envelope(hi)
    assert np.sum(hib - np.arange(nt)) == np.sum(hi - np.arange(nt))          # the same tiles, seen from the other end
    assert _tiles_outside(_factor(name)[::-1, ::-1].T, hib) == []


def test_the_tables_that_are_pinned():
    """clusters_caller: the exact envelope (a cluster of 300, one of 45 and one of 520 sites in this order, every one a
    clique: tile rows 0 .. 2, 2 and 2 .. 6, then the scattered sites); the mirrored envelope of `clusters` is not the
    envelope (the Fisher sweep's second table differs from its first); the stored zero of `lshape` sits where it should."""
    _, nt, hi, W, _ = _envelope("clusters_caller")
    assert hi.tolist() == [8, 8, 10, 10, 10, 10, 10, 10, 11, 11, 11] and W == 8
    _, nt, hi, W, _ = _envelope("clusters")
    assert not np.array_equal(TE.mirrored_envelope(hi), hi)
    for name in ("chain", "hub_caller"):
        hi = _envelope(name)[2]
        assert np.array_equal(TE.mirrored_envelope(hi), hi)
    p = TE.problem("lshape")
    ci, rp, ent = p.ref_taper
    row = 7 * 128 - 1                                   # (nt - 1) 128 - 1: the last row of tile row 6
    assert ci[rp[row] - 1] == 1 and ent[rp[row] - 1] == 0.0 and ci[rp[0 + 1] - 2] == row + 1 and ent[rp[1] - 2] == 0.0
    nt, raw = TE.raw_skyline(p.n, ci, rp, np.arange(1, p.n + 1))
    assert raw[0] == 7
    nt, raw = TE.raw_skyline(p.n, *TE.pattern(p.locs, p.delta)[:2], np.arange(1, p.n + 1))
    assert np.all(raw - np.arange(nt) <= 3)                 # without the zero: a band of three tile rows
    p = TE.problem("hub")
    ci, rp, ent = p.ref_taper
    near = int(np.sum(np.hypot(*(p.locs - p.locs[TE.HUB]).T) <= p.delta))
    assert rp[TE.HUB + 1] - rp[TE.HUB] == p.n and np.sum(ent == 0.0) == 2 * (p.n - near) and 1 < near < 200
    nt, raw = TE.raw_skyline(1153, *TE.problem("chain").ref_taper[:2], _envelope("chain")[0])
    assert np.all(raw - np.arange(nt) <= 2)
    nt, raw = TE.raw_skyline(577, *TE.problem("islands").ref_taper[:2], _envelope("islands")[0])
    assert np.all(raw - np.arange(nt) == 1) and TE.problem("islands").ref_taper[0].size == 577


@pytest.mark.parametrize("name", ["clusters", "clusters_caller", "hub_caller"])
def test_containment_notices_an_envelope_one_tile_too_tight(name):
    """Where the pattern (not the floor) decides a column and real entries fill it, a bound one tile lower lets the factor out."""
    order, nt, hi, W, _ = _envelope(name)
    p = TE.problem(name)
    _, raw = TE.raw_skyline(p.n, p.ref_taper[0], p.ref_taper[1], order)
    fl = TE.floor_envelope(nt)
    decided = [c for c in range(nt) if raw[c] == hi[c] > fl[c]]
    assert decided, (raw, hi, fl)
    for c in decided:
        tight = hi.copy()
        tight[c] -= 1
        out = _tiles_outside(_factor(name), tight)
        assert out == [(int(hi[c]) - 1, c)], (c, out)


def _zero_far_tiles(L, cut):
    """(L with every tile (I, J), I - J >= cut, set to zero; the largest entry that went)"""
    T = TE.TILE
    nt = L.shape[0] // T
    out, gone = L.copy(), 0.0
    for J in range(nt):
        for I in range(J + cut, nt):
            blk = out[I * T:(I + 1) * T, J * T:(J + 1) * T]
            gone = max(gone, float(np.abs(blk).max()))
            blk[:] = 0.0
    return out, gone


@pytest.mark.parametrize("name", TE.WIDE)
def test_far_tiles_matter(name):
    """The condition every wide case must meet before it may claim to test anything (a condition on the inputs, not a
    measurement of the library): with the tiles (I, J), I - J >= 8, of the dense numpy factor set to zero -- the tiles no case
    of W <= 8 has -- the quadratic form |L^-1 (z - X beta)|^2 moves by 1e-6 of itself at least (100 x N2LL_RTOL) and the
    stochastic part of the kriging prediction at the case's 200 rows by 1e-8 of its largest value (100 x the bound of
    test_taper_predict_vs_oracle).  The cross-covariances are the CPU oracle's."""
    from scipy.linalg import solve_triangular
    from oracle import oracle as O
    O.build()
    p = TE.problem(name)
    order, nt, hi, W, _ = _envelope(name)
    o = order - 1
    L = _factor(name)
    Lz, gone = _zero_far_tiles(L, TE.FAR)
    ci, rp, ent = p.pred_taper
    C = np.zeros((TE.M_PRED, nt * TE.TILE))
    Cn = np.zeros((TE.M_PRED, p.n))
    Cn[np.repeat(np.arange(TE.M_PRED), np.diff(rp)), ci - 1] = ent * O.cov_rns_taper_pred(p.theta, p.locs, p.lp, p.X, p.Xp, ci, rp,
                                                                                            TE.SMOOTH_LIMITS)
    C[:, :p.n] = Cn[:, o]
    worst_q, worst_s = np.inf, np.inf
    for col in range(p.z.shape[1]):
        res = np.zeros(nt * TE.TILE)
        res[:p.n] = (p.z[:, col] - p.X @ p.theta["mean"])[o]
        y, yz = solve_triangular(L, res, lower=True), solve_triangular(Lz, res, lower=True)
        st = solve_triangular(L, C.T, lower=True).T @ y
        stz = solve_triangular(Lz, C.T, lower=True).T @ yz
        worst_q = min(worst_q, abs(y @ y - yz @ yz) / (y @ y))
        worst_s = min(worst_s, float(np.max(np.abs(st - stz)) / np.max(np.abs(st))))
    print("%s: W %d, largest entry of the tiles at distance >= %d: %.3e of max |L| = %.3g; zeroing them moves the quadratic form "
          "by %.3e of itself and the stochastic part by %.3e of its largest value" % (name, W, TE.FAR, gone / np.abs(L).max(),
                                                                                 np.abs(L).max(), worst_q, worst_s))
    assert W > TE.FAR and gone > 0
    assert worst_q >= QUAD_MOVES, worst_q
    assert worst_s >= KRIGE_MOVES, worst_s


@pytest.mark.parametrize("name", TE.FLAT)
def test_block_rule_tiles_of_a_flat_band_are_zero(name):
    """A flat band's raw skyline reaches W - 1 tile rows; the two-column block rule gives the even column of a block the
    bound of the odd one, so the tiles at distance W - 1 exist in even columns alone, and the true factor has nothing in them.
    They are storage the schedule walks over, not coverage: the outermost tiles with anything in them are at distance W - 2."""
    p = TE.problem(name)
    order, nt, hi, W, _ = _envelope(name)
    _, raw = TE.raw_skyline(p.n, p.ref_taper[0], p.ref_taper[1], order)
    L = _factor(name)
    T = TE.TILE
    outer = [c for c in range(nt) if hi[c] - c == W]
    assert outer and all(c % 2 == 0 for c in outer), outer
    assert np.max(raw - np.arange(nt)) == W - 1
    for c in outer:
        I = c + W - 1
        assert not np.any(L[I * T:(I + 1) * T, c * T:(c + 1) * T]), c
    full = [c for c in range(nt) if hi[c] - c >= W - 1]
    live = [c for c in full if np.any(L[(c + W - 2) * T:(c + W - 1) * T, c * T:(c + 1) * T])]
    print("%s: W %d; columns at reach W %s, all empty at distance W - 1; %d of %d columns at reach >= W - 1 hold entries at "
          "distance W - 2" % (name, W, outer, len(live), len(full)))
    assert len(live) >= 6 and set(outer) <= set(live), (live, full)


@pytest.mark.parametrize("name", TE.WIDE)
def test_wide_patterns_are_a_function_of_delta(name):
    """No stored zero, every pair within delta stored, and no pair within 1e-12 delta of delta: the device's own neighbour
    search (CoconsTaperFit.from_delta, krige_taper_core_delta) must find exactly this pattern, and -- the entries being
    evaluated in its order of operations -- these doubles."""
    p = TE.problem(name)
    kind = TE.KIND_OF[p.base]
    for rows, pt in ((p.locs, p.ref_taper), (p.lp, p.pred_taper)):
        d = TE._distances_device(rows, p.locs)
        assert not np.any(np.abs(d - p.delta) <= 1e-12 * p.delta)
        ci, rp, ent = pt
        stored = np.zeros(d.shape, dtype=bool)
        stored[np.repeat(np.arange(d.shape[0]), np.diff(rp)), ci - 1] = True
        assert np.array_equal(stored, d <= p.delta) and np.all(ent > 0)
        h = d[stored] / p.delta
        want = (1 - h) ** 2 * (1 + h / 2) if kind == "sph" else (1 - h) ** 4 * (4 * h + 1)
        assert np.allclose(ent, want, rtol=0, atol=4e-16)


@pytest.mark.parametrize("name", TE.NAMES)
def test_prediction_sets(name):
    p = TE.problem(name)
    ci, rp, ent = p.pred_taper
    dense, empty, on_top = p.special
    assert p.lp.shape == (TE.M_PRED, 2) and rp.size == TE.M_PRED + 1 and rp[-1] == ci.size + 1
    assert len({dense // 64, empty // 64, on_top // 64}) == 3
    cnt = np.diff(rp)
    assert cnt[empty] == 0
    assert np.any(np.all(p.locs == p.lp[on_top], axis=1)) and 1.0 in ent[rp[on_top] - 1:rp[on_top + 1] - 1]
    assert cnt[dense] >= (1 if name == "islands" else max(1, np.median(cnt)))      # next to the site with the most neighbours
    for i in range(TE.M_PRED):
        assert np.all(np.diff(ci[rp[i] - 1:rp[i + 1] - 1]) > 0)
    if name.startswith("clusters"):
        assert cnt[dense] >= 520                                # inside the largest cluster: all of it is in range
        pos = np.empty(p.n, dtype=int)
        pos[_envelope(name)[0] - 1] = np.arange(p.n)
        tiles = np.unique(pos[ci[rp[dense] - 1:rp[dense + 1] - 1] - 1] // TE.TILE)
        print("%s: the row inside the largest cluster has neighbours in tile columns %s" % (name, tiles.tolist()))
        assert tiles.size >= 3
    if name == "islands":
        assert cnt.max() <= 3                                   # sites 0.032 apart at least, range 0.03


@pytest.mark.parametrize("name", TE.NAMES)
def test_patterns_are_what_the_library_accepts(name):
    """1-based CSR, symmetric, diagonal stored with taper 1, columns ascending, entries in [0, 1]; stored zeros only where the
    case has them"""
    p = TE.problem(name)
    ci, rp, ent = p.ref_taper
    n = p.n
    rows = np.repeat(np.arange(n), np.diff(rp))
    A = np.full((n, n), -1.0)
    A[rows, ci - 1] = ent
    assert rp[0] == 1 and rp[-1] == ci.size + 1 and np.array_equal(A, A.T)
    assert np.all(np.diag(A) == 1.0) and np.all(ent >= 0) and np.all(ent <= 1)
    for i in range(n):
        assert np.all(np.diff(ci[rp[i] - 1:rp[i + 1] - 1]) > 0)
    zeros = int(np.sum(ent == 0.0))
    assert (zeros > 0) == (name in ("hub", "hub_caller", "lshape")), zeros
    if name == "islands":
        assert ci.size == n


@pytest.mark.parametrize("name", TE.NAMES)
def test_ring_load_rule_at_the_cases_band(name):
    """krige_taper_reference.load_schedule at the case's (nt, W): every tile column enters the ring once, into the slot the
    tile column W places earlier has left, before the first step that updates it and within reach of it.  W = 6, 7 and 8 of
    nt = 11, 8 and 11 do not divide nt: the ring wraps on a boundary of its own."""
    _, nt, hi, W, packed = _envelope(name)
    loads = load_schedule(nt, W)
    assert sorted(I for _, I in loads) == list(range(nt))
    at = dict((I, J) for J, I in loads)
    for J, I in loads:
        if J > 0:
            assert I == J + W - 1 and I % W == (J - 1) % W
    for J in range(nt):
        for I in range(J + 1, int(hi[J])):
            assert at[I] <= J and I <= J + W - 1
    if name in ("clusters", "clusters_caller", "hub", "lshape"):
        assert packed and nt % W != 0


def test_theta_and_design_are_the_workloads():
    from cocons_amd import workloads as wl
    th = wl.theta_full(scale0=np.log(0.2))
    mine = TE.theta_full()
    assert list(mine) == list(th) and all(np.array_equal(mine[k], th[k]) for k in th if k != "mean")
    assert TE.SMOOTH_LIMITS == wl.SMOOTH_LIMITS
    locs = TE.problem("islands").locs
    assert np.allclose(TE.design(locs), wl.design_from_locs(locs)["std.covs"], rtol=0, atol=1e-14)
    wide = TE.wide_theta()
    assert list(wide) == list(mine)
    for k in mine:
        same = np.array_equal(wide[k], mine[k])
        assert same == (k not in ("scale", "nugget")) and np.array_equal(wide[k][1:], mine[k][1:])
    assert all(TE.problem(name).theta["scale"][0] == np.log(0.6) for name in TE.WIDE)


def test_restated_order_on_a_path_and_two_components():
    """rcm_order by hand: a path 2 - 0 - 1 - 3 and an isolated vertex 4.  Components in (degree, index) order of their
    least vertex: {4} first; the path starts at vertex 2 (degree 2 with its diagonal, the smaller index of the two ends), one
    sweep ends in 3, the sweep from 3 gives 3 1 0 2; reversed: 2 0 1 3 4."""
    edges = [(0, 1), (0, 2), (1, 3)]
    stored = np.eye(5, dtype=bool)
    for i, j in edges:
        stored[i, j] = stored[j, i] = True
    ci, rp, _ = TE._csr(stored, np.ones((5, 5)))
    assert TE.rcm_order(5, ci, rp).tolist() == [3, 1, 2, 4, 5]
    nt, hi, W, packed = TE.envelope_of(5, ci, rp, np.arange(1, 6))
    assert (nt, hi.tolist(), W, packed) == (1, [1], 1, False)


# --------------------------------------------------------------------------- the library's rule itself (band_plan.hpp)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def band_plan_exe(tmp_path_factory):
    """tests/band_plan_main.cpp over cocons_amd/csrc/band_plan.hpp, by the host compiler alone (a missing compiler fails)"""
    exe = str(tmp_path_factory.mktemp("band_plan") / "band_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "cocons_amd", "csrc"),
                           os.path.join(ROOT, "tests", "band_plan_main.cpp"), "-o", exe])
    return exe


def _run_band_plan(exe, path, text):
    with open(path, "w") as fh:
        fh.write(text)
    out = {}
    for line in subprocess.check_output([exe, str(path)]).decode().splitlines():
        name, *vals = line.split()
        out[name] = [int(v) for v in vals]
    return out


def _pattern_in_order(p, order):
    """the case's full pattern as the handle keeps it: position i holds observation order[i], columns mapped likewise (within
    a row in the caller's sequence, as the library leaves them)"""
    ci, rp, _ = p.ref_taper
    o = np.asarray(order) - 1
    pos = np.empty(p.n, dtype=np.int64)
    pos[o] = np.arange(p.n)
    cnt = np.diff(rp)[o]
    prp = np.concatenate([[1], 1 + np.cumsum(cnt)])
    pci = np.concatenate([pos[ci[rp[r] - 1:rp[r + 1] - 1] - 1] + 1 for r in o])
    return prp, pci


def _prefix(reach):
    return np.concatenate([[0], np.cumsum(reach)]).tolist()


PINNED = {"clusters": ([5, 5, 6, 6, 10, 10, 10, 10, 11, 11, 11], [3, 7, 7, 7, 7, 9, 11, 11, 11, 11, 11]),
          "hub_caller": ([8] * 8, [8] * 8)}


@pytest.mark.parametrize("name", TE.NAMES)
def test_library_rule_is_the_restated_rule(name, band_plan_exe, tmp_path):
    p = TE.problem(name)
    order, nt, hi, W, _ = _envelope(name)
    prp, pci = _pattern_in_order(p, order)
    got = _run_band_plan(band_plan_exe, tmp_path / "pattern.txt",
                         "%d\n%s\n%s\n" % (p.n, " ".join(map(str, prp.tolist())), " ".join(map(str, pci.tolist()))))
    hib = TE.mirrored_envelope(hi)
    cols = np.arange(nt)
    print("%s: hi %s hib %s" % (name, got["hi"], got["hib"]))
    assert got["status"] == [0]
    assert got["nt"] == [nt] and got["maxband"] == [W] and got["W"] == [W]
    assert got["envelope"] == hi.tolist() and got["hi"] == hi.tolist()
    assert got["hib"] == hib.tolist()
    assert got["toff"] == _prefix(hi - cols) and got["toffb"] == _prefix(hib - cols)
    assert len(got["toff"]) == nt + 1 and got["toff"][nt] == got["toffb"][nt]
    if name in PINNED:
        assert (got["hi"], got["hib"]) == PINNED[name]


def test_library_plan_without_an_envelope(band_plan_exe, tmp_path):
    """a handle without an envelope (COCONS_TAPER_BAND=0) on the tile columns of `clusters`: every column reaches the last
    tile row, the ring holds all of them"""
    nt = _envelope("clusters")[1]
    got = _run_band_plan(band_plan_exe, tmp_path / "none.txt", "0 %d\n" % nt)
    assert got["status"] == [0] and got["nt"] == [nt] and got["W"] == [nt] and got["envelope"] == []
    assert got["hi"] == [nt] * nt and got["hib"] == [nt] * nt
    assert got["toff"] == _prefix(nt - np.arange(nt)) and got["toffb"] == got["toff"]


# --------------------------------------------------------------------------- the bucket sort of tapered kriging (band_buckets)
def _buckets(nt, inv, ci, rp, row0, nrows, stride):
    """band_buckets restated: the entries of rows [row0, row0 + nrows) of the 1-based CSR (ci, rp), numbered from the chunk's
    first entry; hci = 1-based position of an entry's column (inv[caller's column]); the entries stably sorted by the tile
    column of that position (rows in order, a row's entries in the caller's order); hdst = row in the chunk + (position mod
    128) * stride; boff = where each tile column's bucket starts, nt + 1 entries."""
    ci, rp, inv = np.asarray(ci, dtype=np.int64), np.asarray(rp, dtype=np.int64), np.asarray(inv, dtype=np.int64)
    e0, e1 = rp[row0] - 1, rp[row0 + nrows] - 1
    pos = inv[ci[e0:e1] - 1]
    row = np.repeat(np.arange(nrows), np.diff(rp[row0:row0 + nrows + 1]))
    hsrc = np.argsort(pos // TE.TILE, kind="stable")
    hdst = row[hsrc] + (pos[hsrc] % TE.TILE) * stride
    boff = np.concatenate([[0], np.cumsum(np.bincount(pos // TE.TILE, minlength=nt))])
    return {"hci": (pos + 1).tolist(), "hdst": hdst.tolist(), "hsrc": hsrc.tolist(), "boff": boff.tolist()}


def _csr_rows(rows):
    """1-based CSR of a list of rows, each a list of 1-based columns"""
    rp = np.concatenate([[1], 1 + np.cumsum([len(r) for r in rows])]).astype(int)
    return [c for r in rows for c in r], rp.tolist()


def _bucket_cases():
    rng = np.random.default_rng(5)
    n = 300                                     # nt = 3 tile columns, the last one partial
    ident = np.arange(n)
    perm = rng.permutation(n)
    inv128 = ident.copy()                       # caller's columns 1 and 2 at positions 127 and 128: the tile boundary in one row
    inv128[[0, 127]], inv128[[1, 128]] = inv128[[127, 0]], inv128[[128, 1]]
    rows = [sorted(rng.choice(n, size=k, replace=False) + 1) for k in rng.integers(1, 40, size=70)]
    rows[9] = []                                # an empty row inside a chunk
    rows[64], rows[65], rows[66] = [], [], []   # a chunk with no entries at all
    rows[3] = [1, 2, 200]
    m = len(rows)
    return {
        "nt1": (1, np.arange(100), [[5, 7], [], [1, 100]], 0, 3, 64),
        "whole_identity": (3, ident, rows, 0, m, 128),
        "empty_chunk": (3, perm, rows, 64, 3, 64),
        "empty_row_inside": (3, perm, rows, 0, 64, 64),
        "tile_boundary": (3, inv128, rows, 0, 64, 64),
        "permuted": (3, perm, rows, 0, 64, 64),
        "last_short_chunk": (3, perm, rows, 64, m - 64, 64),        # row0 > 0 and nrows = 6 < stride
        "joint_m65": (3, perm, rows[:65], 0, 65, 128),               # stride = round_up(65, 64)
    }


@pytest.mark.parametrize("name", sorted(_bucket_cases()))
def test_library_bucket_sort_is_the_restated_sort(name, band_plan_exe):
    nt, inv, rows, row0, nrows, stride = _bucket_cases()[name]
    ci, rp = _csr_rows(rows)
    text = " ".join(map(str, [nt, len(inv)] + list(inv) + [len(rows)] + rp + ci + [row0, nrows, stride]))
    got = {}
    for line in subprocess.check_output([band_plan_exe, "buckets"], input=text.encode()).decode().splitlines():
        key, *vals = line.split()
        got[key] = [int(v) for v in vals]
    want = _buckets(nt, inv, ci, rp, row0, nrows, stride)
    ne = rp[row0 + nrows] - rp[row0]
    print("%s: %d entries, boff %s" % (name, ne, got["boff"]))
    assert got == want
    # what the device relies on: every entry once, every destination inside the slot's rows [0, nrows) x 128 columns
    assert sorted(got["hsrc"]) == list(range(ne)) and len(got["boff"]) == nt + 1 and got["boff"][-1] == ne
    assert all(0 <= d % stride < max(nrows, 1) and d // stride < TE.TILE for d in got["hdst"])
    if name == "empty_chunk":
        assert ne == 0 and got["boff"] == [0] * (nt + 1)
    if name == "tile_boundary":
        k127, k128 = rp[3] - 1, rp[3]                                       # row 3's first two entries: positions 127 and 128
        assert (got["hci"][k127], got["hci"][k128]) == (128, 129)
        assert got["hsrc"].index(k127) < got["boff"][1] <= got["hsrc"].index(k128)
        assert got["hdst"][got["hsrc"].index(k127)] == 3 + 127 * stride and got["hdst"][got["hsrc"].index(k128)] == 3
