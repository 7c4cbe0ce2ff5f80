"""The maxmin ordering on the device (cocons_vecchia_order) against the sequential greedy of its rule in numpy
(tests/order_reference.py).  Every comparison is array_equal: the worst deviation allowed is 0.  Lines "order-report ..." carry
the cases, the level counts and the work (tests/golden/VECCHIA_ORDER_REPORT.md)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import order_reference as OR  # noqa: E402

pytestmark = pytest.mark.gpu

SETS = list(OR.point_sets()) + ["uniform 20000"]


def _phases(locs, binned_from=0):
    """(order, counts, ms4, stats5) of cocons_debug_order_phases"""
    from cocons_amd import _lib
    L = _lib.load()
    locs = np.asfortranarray(locs, dtype=np.float64)
    n = locs.shape[0]
    order, counts = np.zeros(n, dtype=np.int32), np.zeros(67, dtype=np.int32)
    ms, st = np.zeros(4), np.zeros(5, dtype=np.int64)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    rc = L.cocons_debug_order_phases(n, locs.ctypes.data_as(_lib.c_dp), 0, int(binned_from), ip(order), ip(counts),
                                     ms.ctypes.data_as(_lib.c_dp), st.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    assert rc == 0, _lib.last_error()
    return order, counts[1:1 + counts[0]].copy(), ms, st


@pytest.mark.parametrize("name", SETS)
def test_order_and_level_counts_equal_the_greedy(name):
    from cocons_amd import host
    locs, want, want_counts = OR.reference(name)
    got, counts = host.vecchia_order_device(locs, levels=True)
    off = int(np.count_nonzero(got != want))
    print("order-report gpu | %s | n %d | levels %s | positions that differ %d" % (name, locs.shape[0], counts.tolist(), off))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(counts, want_counts) and int(counts.sum()) == locs.shape[0]
    # without the counts: the same order
    assert np.array_equal(host.vecchia_order_device(locs), want)


@pytest.mark.parametrize("name", SETS)
def test_property_holds_on_the_device_output(name):
    from cocons_amd import host
    locs = OR.reference(name)[0]
    got, counts = host.vecchia_order_device(locs, levels=True)
    worst = OR.check_property(locs, got, counts)          # from d2 values alone: no reference order enters
    print("order-report gpu | %s | largest M_t / m_t %.4f (< 4)" % (name, worst))
    assert worst < 4.0


@pytest.mark.parametrize("name", ["uniform 641", "lattice / 39", "two clusters", "uniform 20000"])
def test_two_calls_give_equal_bits(name):
    from cocons_amd import host
    locs = OR.reference(name)[0]
    a, ca = host.vecchia_order_device(locs, levels=True)
    b, cb = host.vecchia_order_device(locs, levels=True)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)


def test_the_switch_between_the_grids_is_exercised():
    # n = 20 000: some levels on the dense grid, some on the binned one, more than one workgroup per launch
    locs, want, want_counts = OR.reference("uniform 20000")
    got, counts, ms, st = _phases(locs)
    print("order-report gpu | uniform 20000 | levels %d dense %d rounds %d launches %d reads %d | ms %s"
          % (st[0], st[1], st[2], st[3], st[4], np.round(ms, 3).tolist()))
    assert np.array_equal(got, want) and np.array_equal(counts, want_counts)
    assert 0 < st[1] < st[0] and st[0] == want_counts.size - 2
    # two far clusters: the levels beyond the dense grid's cap
    locs, want, want_counts = OR.reference("two clusters")
    got, counts, ms, st = _phases(locs)
    assert np.array_equal(got, want) and 0 < st[1] < st[0]


@pytest.mark.parametrize("name", ["uniform 300", "uniform 5000", "lattice / 39", "lattice, every point twice"])
def test_binned_schedule_from_level_one_gives_the_same_bits(name):
    locs, want, want_counts = OR.reference(name)
    for binned_from in (1, 4):
        got, counts, ms, st = _phases(locs, binned_from)
        print("order-report gpu | %s | binned from level %d | levels %d dense %d rounds %d launches %d | differ %d"
              % (name, binned_from, st[0], st[1], st[2], st[3], int(np.count_nonzero(got != want))))
        assert st[1] == min(binned_from - 1, st[0])
        assert np.array_equal(got, want) and np.array_equal(counts, want_counts)
