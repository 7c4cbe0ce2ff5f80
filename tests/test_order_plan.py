"""The plan of the maxmin ordering without a GPU: cocons_debug_order_plan computes the labels, the centre, L and
every level's (l_k, e_k) with the header the kernels use, and they are numpy's to the bit."""
import numpy as np
import pytest

import order_reference as OR


def _boxes():
    rng = np.random.default_rng(OR.KR.SEED + 7)
    u = rng.uniform(-3.0, 5.0, size=(257, 2))
    return {
        "L = 0": np.tile([[0.3, -0.4]], (7, 1)),
        "one row of cells (all y equal)": np.column_stack([rng.uniform(0, 1, 100), np.full(100, 2.5)]),
        "1e6 times wider than high": u * np.array([1e6, 1.0]),
        "far from the origin": 1e12 + rng.uniform(0, 1, size=(50, 2)),
        "tiny": rng.uniform(0, 1, size=(50, 2)) * 1e-200,
    }


@pytest.mark.parametrize("n", OR.LABEL_SIZES)
def test_plan_labels_and_levels_for_uniform_points(n):
    locs = OR.uniform(n)
    got = OR.plan(locs)
    c, L, lv = OR.geometry(locs)
    assert np.array_equal(got["labels"], OR.labels(n))
    assert np.array_equal(got["centre"], c) and got["L"] == L
    assert np.array_equal(got["levels"], np.asarray(lv))


@pytest.mark.parametrize("name", list(_boxes()))
def test_plan_geometry_of_special_boxes(name):
    locs = _boxes()[name]
    got = OR.plan(locs)
    c, L, lv = OR.geometry(locs)
    assert np.array_equal(got["centre"], c) and got["L"] == L
    assert np.array_equal(got["levels"], np.asarray(lv))
    assert np.array_equal(got["labels"], OR.labels(locs.shape[0]))
    if name == "L = 0":
        assert L == 0.0 and not got["levels"].any()
    else:
        assert got["levels"][0, 0] == L and got["levels"][1, 1] * 4.0 == got["levels"][0, 1]
