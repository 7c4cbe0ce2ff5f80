"""The grouped handle made on the device (cocons_fit_create_vecchia_grouped_knn) against the host route on the
same data: cocons_vecchia_neighbours -> cocons_vecchia_group_rounds -> cocons_vecchia_group_table -> cocons_fit_create_vecchia
-> cocons_vecchia_set_groups.  The exported partition and table agree as integers, cocons_vecchia_info and
cocons_vecchia_groups_info agree, and the grouped value, gradient, whitening and simulation agree to the BIT at one theta in
the Bessel branch (np.array_equal throughout).  Lines "vecchia-group-device-report ..." carry the cases."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CASES = [(2, 30), (65, 30), (641, 30), (641, 10), (3000, 30)]
CAPS = (17, 64)


@functools.lru_cache(maxsize=None)
def data(n):
    """(locs, X, theta, z): test_gpu_dense_sizes.problem's recipe without the oracle's matrix (no reference value is needed:
    both sides are the library's)"""
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(6400 + n)
    p = 1 if n < 3 else 3
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n)] + [rng.standard_normal(n) * 0.5 for _ in range(p - 1)]))
    th = OrderedDict((k, np.array(v[:p], dtype=float)) for k, v in wl.theta_full(scale0=np.log(0.2)).items())
    th["mean"] = np.array([0.3, -0.15, 0.2])[:p]
    z = np.asfortranarray(rng.standard_normal((n, 2)))
    for a in (locs, X, z) + tuple(th.values()):
        a.setflags(write=False)
    return locs, X, th, z


@functools.lru_cache(maxsize=None)
def host_route(n, m, cap):
    """(searched table, labels, statistics, expanded table) by the stateless entries"""
    from cocons_amd import host
    nn = host.vecchia_neighbours_device(data(n)[0], m)
    group, st = host.vecchia_group_rounds(nn, cap, stats=True)
    wide = host.vecchia_group_table(nn, group)
    for a in (nn, group, wide):
        a.setflags(write=False)
    return nn, group, st, wide


def _host_fit(n, m, cap):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = data(n)
    nn, group, st, wide = host_route(n, m, cap)
    g = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    g.set_groups(group)
    return g


def _device_fit(n, m, cap, **more):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = data(n)
    return ca.CoconsVecchiaFit.from_groups_knn(locs, X, z, wl.SMOOTH_LIMITS, m, max_rows=cap, **more)


def _flat(v):
    if isinstance(v, dict):
        return [x for k in sorted(v) for x in _flat(v[k])]
    if isinstance(v, (tuple, list)):
        return [x for e in v for x in _flat(e)]
    return [np.asarray(v)]


def _outputs(f, n):
    """every compared entry at the one theta; flat list of arrays"""
    th = data(n)[2]
    rng = np.random.default_rng(8800 + n)
    W, E = np.asfortranarray(rng.standard_normal((n, 5))), np.asfortranarray(rng.standard_normal((n, 4)))
    grouped = f.neg2loglik_core(th, grouped=True)
    plain = f.neg2loglik_core(th)
    assert plain[0] == grouped[0] and np.array_equal(plain[1], grouped[1])          # the same bits on one handle
    return _flat([grouped, f.neg2loglik_grad_core(th, grouped=True), f.whiten_grouped_core(th, W), f.sim_grouped_core(th, E)])


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("n,m", CASES)
def test_handle_is_the_host_routes_handle(n, m, cap):
    nn, group, st, wide = host_route(n, m, cap)
    f, g = _device_fit(n, m, cap), _host_fit(n, m, cap)
    try:
        block, tab = f.groups_export()
        off = (int(np.count_nonzero(block != group)), int(np.count_nonzero(tab != wide)) if tab.shape == wide.shape else -1)
        print("vecchia-group-device-report gpu | grouped knn handle | n%d m%d cap%d | blocks %d rounds %d m_out %d | labels that "
              "differ %d, table entries that differ %d" % (n, m, cap, st["blocks"], st["rounds"], wide.shape[1], off[0], off[1]))
        assert block.dtype == np.int32 and np.array_equal(block, group)
        assert tab.dtype == np.int32 and tab.shape == wide.shape and np.array_equal(tab, wide)
        hb, ht = g.groups_export()
        assert np.array_equal(hb, group) and np.array_equal(ht, wide)               # the read-back itself, on the host route
        assert np.array_equal(f.groups_export(table=False), group)
        assert f.info() == g.info() and f.m == wide.shape[1]
        assert f.groups_info() == g.groups_info()
        gi = f.groups_info()
        assert (gi["blocks"], gi["rows"], gi["pairs"]) == (st["blocks"], st["rows"], st["pairs"])
        want = _outputs(g, n)
        got = _outputs(f, n)
        assert _same(got, want)
        f2 = _device_fit(n, m, cap)                                                  # a second handle beside the first
        try:
            assert _same(_outputs(f2, n), want) and f2.info() == f.info()
            assert _same(_outputs(f, n), want)
        finally:
            f2.close()
    finally:
        f.close()
        g.close()


def test_a_cap_on_the_rounds():
    """max_rounds = 2 through the handle: the partition after two rounds, its table and its plan"""
    from cocons_amd import host
    n, m, cap = 641, 30, 64
    nn = host_route(n, m, cap)[0]
    group = host.vecchia_group_rounds(nn, cap, 2)
    f = _device_fit(n, m, cap, max_rounds=2)
    try:
        block, tab = f.groups_export()
        assert np.array_equal(block, group) and np.array_equal(tab, host.vecchia_group_table(nn, group))
        assert f.groups_info()["blocks"] == int(group.max()) + 1
    finally:
        f.close()


def test_after_the_maxmin_order():
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    n, m = 641, 30
    locs, X, th, z = data(n)
    h = ca.CoconsVecchiaFit.from_maxmin_groups(locs, X, z, wl.SMOOTH_LIMITS, m, max_rounds=2)      # the cap is passed through
    try:
        oh = h.maxmin_order.astype(np.int64) - 1
        assert np.array_equal(h.groups_export(table=False), host.vecchia_group_rounds(host.vecchia_neighbours_device(locs[oh], m), 64, 2))
    finally:
        h.close()
    f = ca.CoconsVecchiaFit.from_maxmin_groups(locs, X, z, wl.SMOOTH_LIMITS, m)
    try:
        o = f.maxmin_order.astype(np.int64) - 1
        assert np.array_equal(f.maxmin_order, host.vecchia_order_device(locs))
        nn = host.vecchia_neighbours_device(locs[o], m)
        group = host.vecchia_group_rounds(nn, 64)
        block, tab = f.groups_export()
        assert np.array_equal(block, group) and np.array_equal(tab, host.vecchia_group_table(nn, group))
        g = ca.CoconsVecchiaFit.from_groups_knn(locs[o], X[o], z[o], wl.SMOOTH_LIMITS, m)
        try:
            assert f.neg2loglik_core(th, grouped=True)[0] == g.neg2loglik_core(th, grouped=True)[0]
        finally:
            g.close()
    finally:
        f.close()


def test_refusals():
    from cocons_amd import _lib, workloads as wl
    L = _lib.load()
    n = 65
    locs, X, th, z = data(n)
    sl = np.asarray(wl.SMOOTH_LIMITS, dtype=float)
    dp = _lib.c_dp

    def create(m=30, max_rows=64, max_rounds=0, device=0, locs_=locs):
        return L.cocons_fit_create_vecchia_grouped_knn(n, 3, 2, None if locs_ is None else np.asfortranarray(locs_).ctypes.data_as(dp),
                                                       X.ctypes.data_as(dp), z.ctypes.data_as(dp), sl.ctypes.data_as(dp), device, m,
                                                       max_rows, max_rounds)

    who = "cocons_fit_create_vecchia_grouped_knn: "
    for kw, message in (({"m": 0}, "m = 0 is outside 1 .. 63"), ({"m": 64}, "m = 64 is outside 1 .. 63"),
                        ({"max_rows": 1}, "max_rows = 1 is outside 2 .. 64"), ({"max_rows": 65}, "max_rows = 65 is outside 2 .. 64"),
                        ({"max_rounds": -1}, "max_rounds = -1 (0 = 256 rounds at the most)"), ({"locs_": None}, "null argument")):
        assert create(**kw) is None and _lib.last_error() == who + message, (kw, _lib.last_error())
    # the read-back: a handle without a plan, null arguments
    import cocons_amd as ca
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, 10)
    try:
        block = np.full(n, 7, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        assert L.cocons_vecchia_groups_export(f._h, block.ctypes.data_as(ip), None) == -1
        assert _lib.last_error().startswith("cocons_vecchia_groups_export: the handle has no plan")
        assert L.cocons_vecchia_groups_export(f._h, None, None) == -1 and _lib.last_error() == "cocons_vecchia_groups_export: null argument"
        assert L.cocons_vecchia_groups_export(None, block.ctypes.data_as(ip), None) == -1
        assert _lib.last_error() == "cocons_vecchia_groups_export: null fit handle"
        assert np.all(block == 7)
    finally:
        f.close()
    # a device that does not exist; the refusal is that call's alone, the next launch does not find its error
    assert create(device=4096) is None and "invalid device" in _lib.last_error()
    g = ca.CoconsVecchiaFit.from_groups_knn(locs, X, z, wl.SMOOTH_LIMITS, 10)
    try:
        assert g.groups_info()["blocks"] >= 1 and np.isfinite(g.neg2loglik_core(th, grouped=True)[0])
    finally:
        g.close()
