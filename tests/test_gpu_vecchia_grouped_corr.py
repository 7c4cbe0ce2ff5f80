"""The grouped handle on a correlation table made on the device (cocons_fit_create_vecchia_grouped_corr_knn)
against the host route on the same data: cocons_vecchia_neighbours_corr -> cocons_vecchia_group_rounds ->
cocons_vecchia_group_table -> cocons_fit_create_vecchia -> cocons_vecchia_set_groups.  The exported partition and table agree
as integers, and the value, the grouped value, the grouped gradient, a whitening and an unwhitening agree to the BIT
(np.array_equal throughout); the refusals that need a device."""
import functools

import numpy as np
import pytest

import corr_knn_reference as CR

pytestmark = pytest.mark.gpu

SHAPES = ((5, 2, 5), (30, 2, 30))          # (m_cand, hops, m)
CAPS = (64, 2)


@functools.lru_cache(maxsize=None)
def data(n):
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(7100 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(wl.design_from_locs(locs)["std.covs"]) if n > 2 else np.ones((n, 1), order="F")
    th = dict(CR.theta_covariate(), mean=np.array([0.3, -0.15, 0.2])) if n > 2 else dict(CR.theta_aniso(3.0), mean=np.array([0.3]))
    z = np.asfortranarray(rng.standard_normal((n, 2)))
    for a in (locs, X, z):
        a.setflags(write=False)
    return locs, X, th, z


def _host_fit(n, mc, hops, m, cap, max_rounds=0):
    """the host route's handle, and its integers"""
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    locs, X, th, z = data(n)
    f0 = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, 1)
    try:
        nn = f0.neighbours_corr(th, m, m_cand=mc, hops=hops)
    finally:
        f0.close()
    group = host.vecchia_group_rounds(nn, cap, max_rounds)
    wide = host.vecchia_group_table(nn, group)
    g = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    g.set_groups(group)
    return g, group, wide


def _flat(v):
    if isinstance(v, (tuple, list)):
        return [x for e in v for x in _flat(e)]
    return [np.asarray(v)]


def _outputs(f, n):
    th = data(n)[2]
    rng = np.random.default_rng(9900 + n)
    W, E = np.asfortranarray(rng.standard_normal((n, 3))), np.asfortranarray(rng.standard_normal((n, 2)))
    return _flat([f.neg2loglik_core(th), f.neg2loglik_core(th, grouped=True), f.neg2loglik_grad_core(th, grouped=True),
                  f.whiten_core(th, W), f.whiten_grouped_core(th, W), f.unwhiten_core(th, E), f.unwhiten_grouped_core(th, E)])


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("mc,hops,m", SHAPES)
@pytest.mark.parametrize("n", (2, 65, 700))
def test_handle_is_the_host_routes_handle(n, mc, hops, m, cap):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = data(n)
    g, group, wide = _host_fit(n, mc, hops, m, cap)
    f = ca.CoconsVecchiaFit.from_groups_corr_knn(locs, X, z, wl.SMOOTH_LIMITS, th, m, m_cand=mc, hops=hops, max_rows=cap)
    try:
        block, tab = f.groups_export()
        print("vecchia-grouped-corr-report gpu | n%d m_cand%d hops%d m%d cap%d | blocks %d m_out %d | labels that differ %d, "
              "table entries that differ %d" % (n, mc, hops, m, cap, int(group.max()) + 1, wide.shape[1],
                                                int(np.count_nonzero(block != group)),
                                                int(np.count_nonzero(tab != wide)) if tab.shape == wide.shape else -1))
        assert block.dtype == np.int32 and np.array_equal(block, group)
        assert tab.dtype == np.int32 and tab.shape == wide.shape and np.array_equal(tab, wide)
        assert f.info() == g.info() and f.m == wide.shape[1]
        assert f.groups_info() == g.groups_info()
        want, got = _outputs(g, n), _outputs(f, n)
        assert len(got) == len(want) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want))
    finally:
        f.close()
        g.close()


def test_a_cap_on_the_rounds_and_after_the_maxmin_order():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 700
    locs, X, th, z = data(n)
    g, group, wide = _host_fit(n, 30, 2, 30, 64, max_rounds=2)
    g.close()
    f = ca.CoconsVecchiaFit.from_groups_corr_knn(locs, X, z, wl.SMOOTH_LIMITS, th, 30, m_cand=30, hops=2, max_rounds=2)
    try:
        block, tab = f.groups_export()
        assert np.array_equal(block, group) and np.array_equal(tab, wide)
    finally:
        f.close()
    h = ca.CoconsVecchiaFit.from_maxmin_groups_corr(locs, X, z, wl.SMOOTH_LIMITS, th, 10, m_cand=20, hops=2)
    try:
        o = h.maxmin_order.astype(np.int64) - 1
        k = ca.CoconsVecchiaFit.from_groups_corr_knn(locs[o], X[o], z[o], wl.SMOOTH_LIMITS, th, 10, m_cand=20, hops=2)
        try:
            assert all(np.array_equal(u, v) for u, v in zip(h.groups_export(), k.groups_export()))
            assert h.neg2loglik_core(th, grouped=True)[0] == k.neg2loglik_core(th, grouped=True)[0]
        finally:
            k.close()
    finally:
        h.close()


def test_refusals_that_need_a_device():
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    locs, X, th, z = data(65)
    name = "cocons_fit_create_vecchia_grouped_corr_knn"
    big = {k: np.array(v, dtype=float) for k, v in th.items()}
    big["std.dev"][0] = 1500.0
    with pytest.raises(_lib.CoconsHipError, match=name + ": row 2 "):
        ca.CoconsVecchiaFit.from_groups_corr_knn(locs, X, z, wl.SMOOTH_LIMITS, big, 4, m_cand=5, hops=2)
    # and the next handle is made as if nothing had happened
    f = ca.CoconsVecchiaFit.from_groups_corr_knn(locs, X, z, wl.SMOOTH_LIMITS, th, 4, m_cand=5, hops=2)
    f.close()
