"""The Vecchia neighbour search on the device (cocons_vecchia_neighbours) against the numpy brute force of its
rule -- the m candidates with the smallest key (d2, index), d2 = fl(fl(dx dx) + fl(dy dy)), no square root, ties to the
lower index, rows nearest first and zero-padded (tests/knn_reference.py).  Every comparison is array_equal: the worst
deviation allowed is 0.  Lines "knn-report ..." carry the cases and the level counts (tests/golden/VECCHIA_KNN_REPORT.md)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_reference as KR  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 64, 65, 300, 641)
MS = (1, 10, 30, 63)


def _report(what, case, locs, rows_off):
    print("knn-report gpu | %s | %s | levels %d | rows that differ %d" % (what, case, len(KR.plan(locs)["levels"]), rows_off))


def _rows_off(got, want):
    assert got.shape == want.shape and got.dtype == np.int32
    return int(np.count_nonzero(np.any(got != want, axis=1)))


@functools.lru_cache(maxsize=None)
def brute63(n):
    """the m = 63 table of the uniform sites; the table for m is its first m columns (the rule's prefix property)"""
    nn = KR.brute_self(KR.uniform(n), 63)
    nn.setflags(write=False)
    return nn


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_self_search_equals_brute_force(n, m):
    from cocons_amd import host
    locs = KR.uniform(n)
    want = np.asfortranarray(brute63(n)[:, :m])
    got = host.vecchia_neighbours_device(locs, m)
    off = _rows_off(got, want)
    _report("self search", "uniform n%d m%d" % (n, m), locs, off)
    assert np.array_equal(got, want)
    assert np.all(got[0] == 0) and np.all(got[min(n - 1, m)] > 0) == (n > m)


def _orders_5000():
    rng = np.random.default_rng(KR.SEED + 2)
    u = rng.uniform(0, 1, size=(5000, 2))
    corner = u.copy()
    corner[:2500] *= 0.1                      # the first half of the rows in 1 % of the box
    lat = KR.lattice(100, 50)
    blocks = np.vstack([u[:2500] * 1e-3, 1e3 + u[2500:]])      # all of one far cluster first: rows that walk past every cell
    return {"random order": u, "sorted by x": u[np.argsort(u[:, 0], kind="stable")], "corner first": corner,
            "lattice row-major": lat, "lattice permuted": lat[rng.permutation(5000)], "one cluster after the other": blocks}


ORDERS = _orders_5000()


@pytest.mark.parametrize("name", list(ORDERS))
def test_self_search_n5000_m30_in_every_order(name):
    from cocons_amd import host
    locs = ORDERS[name]
    want = KR.brute_self(locs, 30)
    got = host.vecchia_neighbours_device(locs, 30)
    _report("self search", "n5000 m30 %s" % name, locs, _rows_off(got, want))
    assert np.array_equal(got, want)


SPECIAL = KR.special_sets()


@pytest.mark.parametrize("m", (10, 30, 63))
@pytest.mark.parametrize("name", list(SPECIAL))
def test_self_search_on_ties_and_degenerate_boxes(name, m):
    from cocons_amd import host
    locs = SPECIAL[name]
    want = KR.brute_self(locs, m)
    got = host.vecchia_neighbours_device(locs, m)
    _report("self search", "%s n%d m%d" % (name, locs.shape[0], m), locs, _rows_off(got, want))
    assert np.array_equal(got, want)


def test_n300_crosses_three_levels():
    P = KR.plan(KR.uniform(300))
    assert P["head"] == 64 and P["levels"] == [(64, 128), (128, 256), (256, 300)]


@pytest.mark.parametrize("name", ("uniform", "lattice / 39", "collinear", "two clusters", "all coincident", "n = 5"))
def test_plain_knn_equals_brute_force(name):
    from cocons_amd import host
    locs = {"uniform": KR.uniform(641), "n = 5": KR.uniform(5)}.get(name)
    if locs is None:
        locs = SPECIAL[name]
    n = locs.shape[0]
    span = float(np.max(locs.max(axis=0) - locs.min(axis=0)))
    q = KR.queries(locs, 0.05 * span if span > 0 else 0.1, np.random.default_rng(5))      # on observations, 1e12 spans away
    for m in (1, 30, 63):                                  # n = 5: m_pred > n, zero-padded rows
        want = KR.brute_pred(locs, q, m)
        got = host.vecchia_neighbours_pred_device(locs, q, m)
        _report("plain kNN", "%s n%d m%d queries %d" % (name, n, m, q.shape[0]), locs, _rows_off(got, want))
        assert np.array_equal(got, want)
        if m > n:
            assert np.all(got[:, n:] == 0) and np.all(got[:, :n] > 0)
    assert host.vecchia_neighbours_pred_device(locs, np.zeros((0, 2)), 3).shape == (0, 3)


def test_prefix_and_bits():
    from cocons_amd import host
    locs = KR.uniform(641)
    a63, a30 = host.vecchia_neighbours_device(locs, 63), host.vecchia_neighbours_device(locs, 30)
    assert np.array_equal(a30, a63[:, :30])
    assert np.array_equal(a63, host.vecchia_neighbours_device(locs, 63))
    q = KR.queries(locs, 0.05, np.random.default_rng(5))
    p63, p30 = host.vecchia_neighbours_pred_device(locs, q, 63), host.vecchia_neighbours_pred_device(locs, q, 30)
    assert np.array_equal(p30, p63[:, :30])
    assert np.array_equal(p63, host.vecchia_neighbours_pred_device(locs, q, 63))


@pytest.mark.parametrize("name,m", (("uniform", 1), ("uniform", 10), ("uniform", 30), ("uniform", 63), ("uniform 5000", 30),
                                    ("lattice", 30), ("lattice permuted", 30), ("two clusters", 30), ("collinear", 30)))
def test_equals_the_host_search_where_the_two_rules_agree(name, m):
    """np.hypot (host.vecchia_neighbours) and d2 rank near-ties differently; on these inputs the CPU shows first that they do
    not -- the brute force of the rule and the host function agree --, and then the device's table is the host's."""
    from cocons_amd import host
    locs = {"uniform": KR.uniform(641), "uniform 5000": KR.uniform(5000)}.get(name)
    if locs is None:
        locs = SPECIAL[name]
    want = host.vecchia_neighbours(locs, m)
    assert np.array_equal(KR.brute_self(locs, m), want), "the two rules differ on this input: not a case for this test"
    got = host.vecchia_neighbours_device(locs, m)
    _report("self search against host.vecchia_neighbours", "%s n%d m%d" % (name, locs.shape[0], m), locs, _rows_off(got, want))
    assert np.array_equal(got, want)
