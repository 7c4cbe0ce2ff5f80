"""What the tests of the maxmin ordering share: the rule of include/cocons_hip.h as a SEQUENTIAL greedy in
numpy -- the labels, level 0, the walk of every level in ascending label against the smallest d2 to anything taken so far --,
the checker of the property M_t < 4 m_t from d2 values alone, the point sets, and the plan through cocons_debug_order_plan.

d2(a, b) = fl(fl(dx dx) + fl(dy dy)) in fp64.  The greedy keeps near[p] = the smallest d2 from point p to everything taken so
far (a minimum of exact d2 values is exact), so "p conflicts with nothing taken" is near[p] >= e_k: n vector updates of
length n, no tree, no grid, no rounds."""
import ctypes
import functools
import math

import numpy as np

import knn_reference as KR

LEVELS = 64
MIX = (0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35)
LABEL_SIZES = (1, 2, 3, 5, 64, 65, 1000, 2 ** 16, 2 ** 16 + 1)
DBL_MIN = 2.2250738585072014e-308


def labels(n):
    """label(i), i = 0 .. n - 1, in python integers: b-bit words, three multiply-xorshift rounds, cycle walking"""
    b = 1
    while (1 << b) < n:
        b += 1
    mask, s = (1 << b) - 1, (b + 1) // 2

    def mix(v):
        for c in MIX:
            v = (v * c) & mask
            v ^= v >> s
        return v

    out = np.empty(n, dtype=np.int64)
    for i in range(n):
        v = mix(i)
        while v >= n:
            v = mix(v)
        out[i] = v
    return out


def labels_fast(n):
    """the same in uint64 vectors (the products stay below 2^63)"""
    b = 1
    while (1 << b) < n:
        b += 1
    mask, s = np.uint64((1 << b) - 1), np.uint64((b + 1) // 2)

    def mix(v):
        for c in MIX:
            v = (v * np.uint64(c)) & mask
            v = v ^ (v >> s)
        return v

    v = mix(np.arange(n, dtype=np.uint64))
    while np.any(v >= n):
        out = v >= np.uint64(n)
        v[out] = mix(v[out])
    return v.astype(np.int64)


def d2_to(P, q):
    dx, dy = P[:, 0] - q[0], P[:, 1] - q[1]
    return dx * dx + dy * dy


def geometry(locs):
    """(centre, L, [(l_k, e_k) for k = 1 .. 64])"""
    x0, y0 = locs.min(axis=0)
    x1, y1 = locs.max(axis=0)
    L = max(x1 - x0, y1 - y0)
    c = np.array([x0 + 0.5 * (x1 - x0), y0 + 0.5 * (y1 - y0)])
    lv = [(math.ldexp(L, 1 - k), math.ldexp(L, 1 - k) * math.ldexp(L, 1 - k)) for k in range(1, LEVELS + 1)]
    return c, L, lv


def greedy(locs):
    """(order: n int32, 1-based; counts: [level 0, levels 1 .. K, the rest]) by the sequential walk of the rule"""
    locs = np.ascontiguousarray(locs, dtype=np.float64)
    n = locs.shape[0]
    lab = labels_fast(n)
    by_label = np.argsort(lab)                    # by_label[p] = the caller's index with label p
    c, _, lv = geometry(locs)
    first = int(np.argmin(d2_to(locs, c)))        # the first of equal keys: the lower index
    near = d2_to(locs, locs[first])
    free = np.ones(n, dtype=bool)
    free[first] = False
    out, counts = [first], [1]
    for k in range(1, LEVELS + 1):
        if not free.any():
            break
        e = lv[k - 1][1]
        cand = by_label[free[by_label]]           # the unordered points, ascending label
        took = 0
        while True:
            cand = cand[near[cand] >= e]          # whoever conflicts with something taken so far is out for this level
            if cand.size == 0:
                break
            i = int(cand[0])
            out.append(i)
            free[i] = False
            near = np.minimum(near, d2_to(locs, locs[i]))
            near[i] = -1.0                        # taken: never a candidate again (d2 to itself is 0, and e may be 0 too)
            cand = cand[1:]
            took += 1
        counts.append(took)
    rest = by_label[free[by_label]]
    counts.append(int(rest.size))
    return (np.concatenate([np.asarray(out, dtype=np.int64), rest]) + 1).astype(np.int32), np.asarray(counts, dtype=np.int32)


def check_property(locs, order, counts):
    """Asserts that order is a permutation, that the counts sum to n, and M_t < 4 m_t at every position t >= 1 outside the
    rest whose level has a normal e_k (the property's proof needs e_(k-1) = 4 e_k exactly and e_k > 0: with L = 0 every e_k
    is 0, nothing conflicts and level 1 holds all points).  m_t: the smallest d2 from the point at t to the points before it;
    M_t: the largest smallest-d2-to-those-points over the points at or behind t.  Returns the largest M_t / m_t seen."""
    locs = np.ascontiguousarray(locs, dtype=np.float64)
    n = locs.shape[0]
    o = np.asarray(order, dtype=np.int64) - 1
    assert o.shape == (n,) and np.array_equal(np.sort(o), np.arange(n))
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.sum() == n and counts[0] == 1 and np.all(counts >= 0)
    _, _, lv = geometry(locs)
    level_of = np.repeat(np.arange(counts.size), counts)          # per position; the last record is the rest
    P = locs[o]
    near = d2_to(P, P[0])
    worst = 0.0
    for t in range(1, n - int(counts[-1])):
        k = int(level_of[t])
        m_t, M_t = near[t], near[t:].max()
        if lv[k - 1][1] >= DBL_MIN:
            assert M_t < 4.0 * m_t, (t, k, M_t, m_t)
            worst = max(worst, M_t / m_t)
        near = np.minimum(near, d2_to(P, P[t]))
    return worst


def uniform(n):
    return KR.uniform(n)


def sorted_by_x(n):
    u = KR.uniform(n)
    return u[np.argsort(u[:, 0], kind="stable")]


def corner_first(n):
    u = KR.uniform(n)
    return u[np.argsort(u[:, 0] + u[:, 1], kind="stable")]


def far_clusters():
    rng = np.random.default_rng(KR.SEED + 2)
    return np.vstack([rng.uniform(0, 1, size=(150, 2)), 1e12 + rng.uniform(0, 1, size=(150, 2))])[rng.permutation(300)]


def doubled_lattice():
    lat = KR.lattice(12, 12) * 0.37
    rng = np.random.default_rng(KR.SEED + 3)
    return np.vstack([lat, lat])[rng.permutation(2 * lat.shape[0])]


UNIFORM_SIZES = (1, 2, 3, 64, 65, 300, 641, 5000)


def point_sets():
    """name -> locs: every set the issue names but n = 20 000 (cases_large)"""
    sets = {"uniform %d" % n: uniform(n) for n in UNIFORM_SIZES}
    sets["sorted by x 5000"] = sorted_by_x(5000)
    sets["corner first 5000"] = corner_first(5000)
    sets.update(KR.special_sets())
    sets["two clusters 1e12 apart"] = far_clusters()
    sets["lattice, every point twice"] = doubled_lattice()
    return sets


@functools.lru_cache(maxsize=None)
def reference(name):
    """(locs, order, counts) of a named set, computed once per session and shared: do not write into the arrays"""
    locs = uniform(20000) if name == "uniform 20000" else point_sets()[name]
    order, counts = greedy(locs)
    for a in (locs, order, counts):
        a.setflags(write=False)
    return locs, order, counts


def plan(locs):
    """{"labels", "centre", "L", "levels": 64 x 2 (l_k, e_k)} through cocons_debug_order_plan"""
    from cocons_amd import _lib
    L = _lib.load()
    locs = np.asfortranarray(locs, dtype=np.float64)
    n = locs.shape[0]
    lab = np.zeros(n, dtype=np.int32)
    geom, lv = np.zeros(3), np.zeros((LEVELS, 2))
    rc = L.cocons_debug_order_plan(n, locs.ctypes.data_as(_lib.c_dp), lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                   geom.ctypes.data_as(_lib.c_dp), lv.ctypes.data_as(_lib.c_dp))
    assert rc == 0, _lib.last_error()
    return {"labels": lab, "centre": geom[:2].copy(), "L": float(geom[2]), "levels": lv}
