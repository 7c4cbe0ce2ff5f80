"""CoconsVecchiaFit.from_maxmin against from_knn on the arrays permuted by the reference order: value, parts,
whitened columns, gradient and one simulated field TO THE BIT -- the worst deviation allowed is 0 --, and the two helpers
that carry per-row arrays into and out of the handle's order.  Lines "order-report ..." carry the cases
(tests/golden/VECCHIA_ORDER_REPORT.md)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import order_reference as OR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a, b):
    a, b = np.asarray(a, dtype=float).ravel(), np.asarray(b, dtype=float).ravel()
    assert a.shape == b.shape
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return 0.0 if np.all(same) else float(np.max(np.abs(a - b)[~same]))


def _outputs(f, th, B, E):
    v, parts = f.neg2loglik_core(th)
    Y, logd = f.whiten_core(th, B)
    gv, gparts, gt, gq, gm = f.neg2loglik_grad_core(th)
    return {"value": [v], "parts": parts, "whitened": Y, "logd": logd, "grad value": [gv], "grad parts": gparts,
            "grad table": gt, "grad quad": gq, "grad mean": gm, "field": f.sim_core(th, E)}


@pytest.mark.parametrize("m", (1, 30))
@pytest.mark.parametrize("n", (65, 641))
def test_from_maxmin_has_the_bits_of_from_knn_on_the_permuted_arrays(n, m):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    want_order = OR.greedy(locs)[0]
    o = want_order.astype(np.int64) - 1
    E = np.random.default_rng(31 + n).standard_normal((n, 1))
    a = ca.CoconsVecchiaFit.from_maxmin(locs, X, z, wl.SMOOTH_LIMITS, m)
    b = ca.CoconsVecchiaFit.from_knn(locs[o], np.asfortranarray(X[o]), z[o], wl.SMOOTH_LIMITS, m)
    try:
        assert np.array_equal(a.maxmin_order, want_order) and a.m == m and a.info()["n"] == n
        # the helpers: into the handle's order and back
        assert np.array_equal(a.to_maxmin(Rz), Rz[o]) and np.array_equal(a.to_maxmin(locs[:, 0]), locs[o, 0])
        assert np.array_equal(a.from_maxmin_order(a.to_maxmin(Rz)), Rz)
        assert np.array_equal(a.to_maxmin(a.from_maxmin_order(E)), E)
        oa, ob = _outputs(a, th, a.to_maxmin(Rz), a.to_maxmin(E)), _outputs(b, th, Rz[o], E[o])
        field_caller = a.from_maxmin_order(oa["field"])
    finally:
        a.close()
        b.close()
    worst = max(_dev(oa[k], ob[k]) for k in oa)
    print("order-report gpu | from_maxmin against from_knn on the permuted arrays: value parts whitened logd gradient field "
          "| n%d m%d | worst deviation %.1e" % (n, m, worst))
    for k in oa:
        assert np.array_equal(np.asarray(oa[k]), np.asarray(ob[k]), equal_nan=True), k
    assert np.all(np.isfinite(oa["field"])) and np.array_equal(field_caller[o], ob["field"])
