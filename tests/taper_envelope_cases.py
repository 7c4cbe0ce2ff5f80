"""Taper problems whose band envelope is NOT the flat one every other taper test has (test infrastructure; numpy only,
nothing of the library is imported or read), and the envelope rule restated.

A taper handle factors S = T o C(theta) inside a tile envelope hi[c] (one past the last 128-row tile of tile column c) that
the library derives from the caller's pattern in the handle's order.  envelope_of restates that rule, rcm_order the order the
library chooses on its own, mirrored_envelope the envelope of the flipped factor the Fisher sweep builds.  tests/
test_taper_envelope_cases.py holds the restatement against the fill of a dense numpy Cholesky factor; tests/
test_gpu_taper_envelopes.py holds the library against it.

The cases (problem(name) -> Problem): sites, design, theta, observations, the taper pattern `ref_taper` (1-based CSR,
symmetric, diagonal stored, columns ascending) and a prediction set with its pattern.  Wendland-1 taper of range delta.  A
STORED ZERO is an entry of the pattern whose taper value is 0.0: S does not change (it stays positive definite), the
envelope does -- the only way to shape an envelope without touching the matrix.

  clusters         three tight clusters (300, 45 and 520 sites, each inside one taper range) and 416 scattered sites,
                   n = 1281 = 10 x 128 + 1, shuffled; the library's order.  A clique of 520 sites fills 5 tile rows
                   whatever the order; the scattered sites stay at the floor.
  clusters_caller  the same observations cluster by cluster, then the scattered ones by x; the caller's order.
  islands          577 sites, every one farther than delta from every other: S is diagonal, 5 tile columns.
  chain            1153 sites along a serpentine, two neighbours on either side, shuffled: raw envelope of 2.  The control.
  hub              900 uniform sites; site HUB is joined to all others by stored zeros; the library's order.
  hub_caller       the same in the caller's order: every column reaches the last tile row, W = nt, unpacked buffer.
  lshape           897 sites sorted by x and ONE stored zero at row (nt - 1) 128 - 1, column 0; the caller's order.

Bands wider than eight tile rows (tests/golden/WIDE_BANDS_REPORT.md).  These three have a theta of their own (wide_theta: a
longer range and a nugget as large as the variance keep cond(S) at about 500 and the far tiles of the factor audible); the flat ones use
the spherical taper (1 - h)^2 (1 + h / 2), ten times Wendland-1 near h = 0.8, evaluated in the order of operations of the
device's own pattern search so that a handle made from delta alone holds the same doubles.  tests/
test_taper_envelope_cases.py asserts for each that zeroing every tile (I, J), I - J >= 8, of the dense factor moves the
quadratic form and the kriging prediction far above the suite's tolerances: without that a wide case tests nothing.

  flat9            1665 = 13 x 128 + 1 sites on a strip, sorted by x, delta = 0.6, r = 2; the caller's order.  A flat band:
                   raw reach 9, W = 10 by the two-column block rule (the tiles at distance W - 1 exist in even columns only
                   and are structurally zero), six columns at reach W or W - 1.
  flat10_long      2433 = 19 x 128 + 1 sites on the same strip, delta = 0.37; the caller's order.  W = 10 of nt = 20: the ring
                   wraps twice.  Only the entries whose reference is S and one factorisation run on it.
  tall             a clique of 1300 sites in a disc of diameter 0.28 < delta = 0.3 first, then 569 scattered sites by x; the
                   caller's order.  Column 0 is twelve tile rows tall, the scattered columns stay at the floor.
  tall_rcm         the same observations in the library's order (W = 11, the clique behind the scattered sites).
"""
from __future__ import annotations

import functools
from collections import OrderedDict, namedtuple

import numpy as np

TILE = 128
SMOOTH_LIMITS = (0.5, 2.5)
M_PRED = 200


# --------------------------------------------------------------------------- the rules, restated
def raw_skyline(n, colindices, rowpointers, order):
    """Step 1 of the envelope: per tile column c the last tile row + 1 of any row whose first stored column lies in a tile
    column <= c (a row of the factor is non-zero from its first stored column on), at least the diagonal tile.
    order: 1-based observation per position, as CoconsTaperFit.order() reports it (identity: the caller's order)."""
    ci = np.asarray(colindices, dtype=np.int64) - 1
    rp = np.asarray(rowpointers, dtype=np.int64) - 1
    piv = np.asarray(order, dtype=np.int64) - 1
    assert sorted(piv.tolist()) == list(range(n))
    pos = np.empty(n, dtype=np.int64)
    pos[piv] = np.arange(n)
    nt = (n + TILE - 1) // TILE
    rows = pos[np.repeat(np.arange(n), np.diff(rp))]
    first = np.arange(n)
    np.minimum.at(first, rows, pos[ci])
    raw = np.arange(1, nt + 1)
    for i in range(n):
        c0, ti = first[i] // TILE, i // TILE
        raw[c0:ti + 1] = np.maximum(raw[c0:ti + 1], ti + 1)
    return nt, raw


def floor_envelope(nt):
    """What the rule gives a pattern that asks for nothing: the schedule works on blocks of two tile columns and every block
    is given the next diagonal block as well, hi[c] >= min((c & ~1) + 4, nt)."""
    return np.array([min((c & ~1) + 4, nt) for c in range(nt)])


def envelope_of(n, colindices, rowpointers, order):
    """(nt, hi, W, packed): the skyline, the bound per block of two tile columns, the floor, the running maximum;
    W = max(hi[c] - c) tile rows per packed tile column, packed = W < nt."""
    nt, raw = raw_skyline(n, colindices, rowpointers, order)
    hi = np.empty(nt, dtype=np.int64)
    run = 0
    for c in range(nt):
        k = c & ~1
        bound = max(raw[k:k + 2])                       # both columns of the block
        bound = max(bound, min(k + 4, nt))              # the floor
        run = max(run, min(bound, nt))                  # monotone
        hi[c] = run
    W = int(np.max(hi - np.arange(nt)))
    return nt, hi, W, W < nt


def mirrored_envelope(hi):
    """The envelope of the flipped factor (rows and columns reversed, transposed): its tile column nt - 1 - J reaches down to
    the mirror of the first tile column whose envelope holds tile row J."""
    nt = len(hi)
    out = np.empty(nt, dtype=np.int64)
    for J in range(nt):
        lo = min(K for K in range(J + 1) if hi[K] > J)
        out[nt - 1 - J] = nt - lo
    return out


def rcm_order(n, colindices, rowpointers):
    """The order a taper handle chooses by itself, 1-based: reverse Cuthill-McKee.  Components are started from their
    unvisited vertex of least (degree, index); one sweep from it ends in the root (pseudo-peripheral); the sweep from the root
    appends every vertex's unvisited neighbours by (degree, index); the whole list is reversed."""
    ci = np.asarray(colindices, dtype=np.int64) - 1
    rp = np.asarray(rowpointers, dtype=np.int64) - 1
    deg = np.diff(rp)

    def sweep(root, seen):
        out = [root]
        seen[root] = True
        h = 0
        while h < len(out):
            nb = ci[rp[out[h]]:rp[out[h] + 1]]
            nb = np.unique(nb[~seen[nb]])
            seen[nb] = True
            out.extend(nb[np.lexsort((nb, deg[nb]))].tolist())
            h += 1
        return out

    seen = np.zeros(n, dtype=bool)
    order = []
    for start in np.lexsort((np.arange(n), deg)):
        if seen[start]:
            continue
        probe = sweep(int(start), seen)
        seen[probe] = False
        order.extend(sweep(probe[-1], seen))
    return np.asarray(order[::-1], dtype=np.int64) + 1


# --------------------------------------------------------------------------- the problems
def theta_full():
    """cocons_amd.workloads.theta_full(scale0 = log 0.2) with a mean (the CPU test holds the two equal)"""
    th = OrderedDict()
    th["mean"] = np.array([0.3, -0.2, 0.1])
    th["std.dev"] = np.array([0.0, 0.3, -0.2])
    th["scale"] = np.array([np.log(0.2), 0.2, 0.1])
    th["aniso"] = np.array([0.0, 0.25, -0.25])
    th["tilt"] = np.array([0.0, 0.3, 0.3])
    th["smooth"] = np.array([0.0, 0.5, -0.5])
    th["nugget"] = np.array([np.log(1e-2), 0.0, 0.0])
    return th


def shifted(th):
    """another theta on the same handle: the shift of tests/test_gpu_krige_taper.py"""
    out = OrderedDict((k, np.array(v, dtype=float)) for k, v in th.items())
    out["scale"] = out["scale"] + np.array([0.15, 0.0, 0.0])
    out["nugget"] = out["nugget"] + np.array([0.2, 0.0, 0.0])
    return out


def design(locs):
    """[1, x, y], the covariates standardised (cocons_amd.workloads.design_from_locs)"""
    X = np.column_stack([np.ones(locs.shape[0]), locs[:, 0], locs[:, 1]])
    X[:, 1:] = (X[:, 1:] - X[:, 1:].mean(axis=0)) / X[:, 1:].std(axis=0, ddof=1)
    return np.asfortranarray(X)


def _wendland1(d, delta):
    h = np.minimum(d / delta, 1.0)
    return (1.0 - h) ** 4 * (4.0 * h + 1.0)


def _distances(a, b):
    return np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])


def wide_theta():
    """theta of the cases wider than eight tile rows: range intercept log 0.6, nugget intercept log 1 (cond(S) about 500:
    with theta_full's they stand at 2.5e4 .. 4.8e4, and at log 0.45 / log 0.1, cond(S) 4e3, the two routes of the sparse
    prediction still differed by more than the bound the suite holds them to)"""
    th = theta_full()
    th["scale"] = np.array([np.log(0.6), 0.2, 0.1])
    th["nugget"] = np.array([np.log(1.0), 0.0, 0.0])
    return th


def _spherical(d, delta):
    """(1 - h)^2 (1 + h / 2) = 1 - 1.5 h + 0.5 h^3, in the device's order of operations"""
    h = np.minimum(d / delta, 1.0)
    return (1.0 - 1.5 * h) + (0.5 * h) * (h * h)


def _wendland1_device(d, delta):
    """_wendland1 in the device's order of operations"""
    h = np.minimum(d / delta, 1.0)
    u2 = (1.0 - h) * (1.0 - h)
    return (u2 * u2) * (4.0 * h + 1.0)


def _distances_device(a, b):
    """sqrt(dx dx + dy dy), as the device's pattern search forms a distance (hypot may differ in the last bit)"""
    dx, dy = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


# kind: the name the library knows the case's taper by (CoconsTaperFit.from_delta, krige_taper_core_delta); the cases not
# listed are Wendland-1 through hypot, as they always were
KIND_OF = {"flat9": "sph", "flat10_long": "sph", "tall": "wend1"}
_TAPER_OF = {"sph": _spherical, "wend1": _wendland1_device}


def device_pattern(a, b, delta, kind):
    """(colindices, rowpointers, entries) of rows a against columns b as the library's own search states them: d <= delta"""
    d = _distances_device(a, b)
    return _csr(d <= delta, _TAPER_OF[kind](d, delta))


def _csr(stored, values):
    """1-based CSR of the entries marked in `stored`, columns ascending"""
    rows, cols = np.nonzero(stored)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=stored.shape[0]))]) + 1
    return (cols + 1).astype(np.int32), rp.astype(np.int32), values[rows, cols].copy()


def pattern(locs, delta, zeros=()):
    """(colindices, rowpointers, entries): every pair within delta, and the pairs of `zeros` (both orders) -- stored zeros
    where they are farther apart than delta"""
    d = _distances(locs, locs)
    stored = d <= delta
    for i, j in zeros:
        stored[i, j] = stored[j, i] = True
    return _csr(stored, _wendland1(d, delta))


def pred_pattern(lp, locs, delta):
    d = _distances(lp, locs)
    return _csr(d <= delta, _wendland1(d, delta))


Problem = namedtuple("Problem", "name n delta rcm locs X theta z ref_taper lp Xp pred_taper special base perm")
# special = (row inside the densest neighbourhood, row without a neighbour, row on top of an observation)
# base, perm: the case whose observations these are in another order -- observation i here is observation perm[i] there
# (0-based; the case itself and the identity where it stands alone): what is computed per observation is computed once

Case = namedtuple("Case", "name rcm r base")
CASES = [Case("clusters", True, 2, "clusters"), Case("clusters_caller", False, 2, "clusters"),
         Case("islands", True, 1, "islands"), Case("chain", True, 1, "chain"), Case("hub", True, 1, "hub"),
         Case("hub_caller", False, 1, "hub"), Case("lshape", False, 1, "lshape"),
         Case("flat9", False, 2, "flat9"), Case("flat10_long", False, 1, "flat10_long"), Case("tall", False, 1, "tall"),
         Case("tall_rcm", True, 1, "tall")]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
WIDE = ["flat9", "flat10_long", "tall", "tall_rcm"]          # bands wider than eight tile rows
FLAT = ["flat9", "flat10_long"]
FAR = 8                                                      # tiles (I, J), I - J >= FAR: what no narrower case has
TALL_CLIQUE = 1300
HUB = 450            # the hub's index in `hub` / `hub_caller`: neither first nor last


def _cluster_sites(rng):
    """(locs 1281 x 2, label): label 0, 1, 2 the clusters of 300, 45 and 520 sites (discs of diameter 0.09 < delta = 0.1,
    centres farther apart than two taper ranges), 3 the 416 scattered sites"""
    parts, label = [], []
    for k, (size, centre) in enumerate(((300, (0.22, 0.25)), (45, (0.75, 0.2)), (520, (0.6, 0.72)))):
        rad = 0.045 * np.sqrt(rng.uniform(0, 1, size))
        ang = rng.uniform(0, 2 * np.pi, size)
        parts.append(np.column_stack([centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)]))
        label += [k] * size
    parts.append(rng.uniform(0, 1, size=(416, 2)))
    label += [3] * 416
    return np.concatenate(parts), np.array(label)


def _clusters_caller_perm():
    """clusters_caller in terms of clusters: cluster by cluster, then the scattered sites by x"""
    rng = np.random.default_rng(1281)
    locs, label = _cluster_sites(rng)
    shuffle = rng.permutation(locs.shape[0])                  # clusters = these sites shuffled
    where = np.empty_like(shuffle)
    where[shuffle] = np.arange(shuffle.size)
    tail = np.nonzero(label == 3)[0]
    return where[np.concatenate([np.nonzero(label < 3)[0], tail[np.argsort(locs[tail, 0], kind="stable")]])]


def _sites(name):
    """(locs, delta, stored zeros) of a case that stands alone"""
    if name == "clusters":
        rng = np.random.default_rng(1281)
        locs, label = _cluster_sites(rng)
        return locs[rng.permutation(locs.shape[0])], 0.1, ()
    if name == "islands":
        rng = np.random.default_rng(577)
        g = 25                                                # cells of edge 0.04, a site within 0.004 of the centre
        cells = rng.permutation(g * g)[:577]
        centre = np.column_stack([cells % g, cells // g]) / g + 0.5 / g
        return centre + rng.uniform(-0.004, 0.004, size=centre.shape), 0.03, ()
    if name == "chain":
        rng = np.random.default_rng(1153)
        n, step, rows = 1153, 0.004, 6                        # a site every 0.004 along lanes of length 0.9, 0.15 apart,
        lane, rise = 0.9, 0.15                                # joined by straight risers at alternating ends
        t = np.arange(n) * step                               # arc length along the serpentine
        period = lane + rise
        k, u = np.divmod(t, period)
        assert k.max() < rows
        x = np.where(u <= lane, u, lane)
        x = np.where(k % 2 == 0, x, lane - x) + 0.05
        y = 0.05 + rise * k + np.where(u <= lane, 0.0, u - lane)
        return np.column_stack([x, y])[rng.permutation(n)], 0.0101, ()
    if name == "hub":
        locs = np.random.default_rng(900).uniform(0, 1, size=(900, 2))
        return locs, 0.15, tuple((HUB, j) for j in range(900) if j != HUB)
    if name == "lshape":
        locs = np.random.default_rng(897).uniform(0, 1, size=(897, 2))
        locs = locs[np.argsort(locs[:, 0], kind="stable")]
        nt = (897 + TILE - 1) // TILE
        return locs, 0.15, (((nt - 1) * TILE - 1, 0),)
    if name in ("flat9", "flat10_long"):
        n, delta = (1665, 0.6) if name == "flat9" else (2433, 0.37)
        rng = np.random.default_rng(n)
        x = np.sort(rng.uniform(0, 1, n))
        return np.column_stack([x, rng.uniform(0, 0.3, n)]), delta, ()
    if name == "tall":
        rng = np.random.default_rng(1869)
        rad = 0.14 * np.sqrt(rng.uniform(0, 1, TALL_CLIQUE))
        ang = rng.uniform(0, 2 * np.pi, TALL_CLIQUE)
        clique = np.column_stack([0.5 + rad * np.cos(ang), 0.5 + rad * np.sin(ang)])
        rest = rng.uniform(0, 3, size=(569, 2))
        return np.concatenate([clique, rest[np.argsort(rest[:, 0], kind="stable")]]), 0.3, ()
    raise KeyError(name)


# the box the prediction rows are drawn in, where it is not the unit square
_PRED_BOX = {"flat9": (1.0, 0.3), "flat10_long": (1.0, 0.3)}


@functools.lru_cache(maxsize=None)
def problem(name):
    """The named case, from fixed seeds; computed once, every array read-only."""
    c = BY_NAME[name]
    if c.base != name:
        b = problem(c.base)
        perm = _clusters_caller_perm() if name == "clusters_caller" else np.arange(b.n)
        where = np.empty_like(perm)
        where[perm] = np.arange(b.n)
        ci, rp, _ = b.ref_taper
        brow = np.repeat(np.arange(b.n), np.diff(rp))
        far = _distances(b.locs, b.locs)[brow, ci - 1] > b.delta
        zeros = tuple(zip(where[brow[far]].tolist(), where[ci[far] - 1].tolist()))
        locs = b.locs[perm]
        if c.base in KIND_OF:
            assert not zeros
            tapers = device_pattern(locs, locs, b.delta, KIND_OF[c.base]), device_pattern(b.lp, locs, b.delta, KIND_OF[c.base])
        else:
            tapers = pattern(locs, b.delta, zeros), pred_pattern(b.lp, locs, b.delta)
        out = Problem(name, b.n, b.delta, c.rcm, locs, np.asfortranarray(b.X[perm]), b.theta, np.asfortranarray(b.z[perm]),
                      tapers[0], b.lp, b.Xp, tapers[1], b.special, c.base, perm)
        for a in (out.locs, out.X, out.z, perm) + out.ref_taper + out.pred_taper:
            a.setflags(write=False)
        return out
    locs, delta, zeros = _sites(name)
    n = locs.shape[0]
    rng = np.random.default_rng(7000 + n)
    X = design(locs)
    z = np.asfortranarray(rng.standard_normal((n, c.r)))
    kind = KIND_OF.get(name)
    ref_taper = device_pattern(locs, locs, delta, kind) if kind else pattern(locs, delta, zeros)
    deg = np.diff(ref_taper[1] if kind else pattern(locs, delta)[1])
    busiest = int(np.argmax(deg))
    lp = rng.uniform(0, 1, size=(M_PRED, 2)) * np.array(_PRED_BOX.get(name, (1.0, 1.0)))
    special = (70, 4, 133)                                    # rows of three different 64-row chunks
    lp[special[0]] = locs[busiest] + np.array([0.002, -0.001])
    lp[special[1]] = np.array([4.0, 4.0])
    lp[special[2]] = locs[(3 * n) // 7]
    Xp = np.asfortranarray(np.column_stack([np.ones(M_PRED), rng.standard_normal(M_PRED), rng.standard_normal(M_PRED)]))
    pred_taper = device_pattern(lp, locs, delta, kind) if kind else pred_pattern(lp, locs, delta)
    theta = wide_theta() if name in WIDE else theta_full()
    out = Problem(name, n, delta, c.rcm, locs, X, theta, z, ref_taper, lp, Xp, pred_taper, special, name, np.arange(n))
    for a in (locs, X, z, lp, Xp, out.perm) + ref_taper + pred_taper + tuple(out.theta.values()):
        a.setflags(write=False)
    return out


def order_of(prob):
    """the order the handle will take the observations in, 1-based"""
    if prob.rcm:
        return rcm_order(prob.n, prob.ref_taper[0], prob.ref_taper[1])
    return np.arange(1, prob.n + 1)


def take_rows(pt, idx):
    """the rows idx of a prediction pattern"""
    ci, rp, ent = pt
    sel = np.concatenate([np.arange(rp[i] - 1, rp[i + 1] - 1) for i in idx]) if len(idx) else np.zeros(0, dtype=int)
    rp2 = np.concatenate([[1], 1 + np.cumsum((rp[1:] - rp[:-1])[idx])]).astype(np.int32)
    return ci[sel], rp2, ent[sel]


# --------------------------------------------------------------------------- the shapes the cases claim
def interior(nt):
    """tile columns whose floor is not cut off by the matrix's last tile row"""
    return [c for c in range(nt) if (c & ~1) + 4 <= nt]


def assert_shape(name, nt, hi, W, packed):
    """The case's row of the table (module docstring), for an envelope as envelope_of returns it -- applied to the restated
    order on the CPU and to the order the handle reports on the GPU: a changed ordering rule may move tiles, it must not empty
    a case of its meaning."""
    hi = np.asarray(hi)
    reach = hi - np.arange(nt)
    fl = floor_envelope(nt)
    inner = interior(nt)
    assert np.all(hi >= fl) and np.all(np.diff(hi) >= 0) and hi[-1] == nt
    if name == "clusters":
        assert nt == 11 and packed and W >= 6, (nt, W)
        assert sum(hi[c] == fl[c] for c in inner) >= 2, reach
        assert len(set(reach[inner].tolist())) > 1, reach
        assert len(set((hi - fl)[inner].tolist())) > 1, reach          # wide in one place, at the floor in another
    elif name == "clusters_caller":
        assert nt == 11 and packed and W >= 6, (nt, W)
    elif name == "islands":
        assert nt == 5 and packed and W == 4 and np.array_equal(hi, fl), reach
    elif name == "chain":
        assert nt == 10 and packed and W == 4 and np.array_equal(hi, fl), reach
    elif name == "hub":
        assert nt == 8 and packed and W == nt - 1, (nt, W)
    elif name == "hub_caller":
        assert nt == 8 and not packed and W == nt and np.all(hi == nt), reach
    elif name == "lshape":
        assert nt == 8 and packed and W == nt - 1 and hi[0] == nt - 1, reach     # the last tile row is outside column 0
    elif name == "flat9":
        assert nt == 14 and packed and W >= 9, (nt, W)
        assert np.sum(reach >= W - 1) >= 6, reach
    elif name == "flat10_long":
        assert nt == 20 and packed and W >= 10 and nt >= 2 * W, (nt, W)            # the ring wraps twice
        assert np.sum(reach >= W - 1) >= 8, reach
    elif name in ("tall", "tall_rcm"):
        assert nt == 15 and packed and W >= 11, (nt, W)
        assert sum(hi[c] == fl[c] for c in inner) >= 2, reach
        assert not np.array_equal(mirrored_envelope(hi), hi), reach
    else:
        raise KeyError(name)
