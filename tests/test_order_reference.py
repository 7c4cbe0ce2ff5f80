"""The references of the maxmin ordering held to each other without a GPU: the labels are a permutation, the
sequential greedy of order_reference.py returns a permutation with the property M_t < 4 m_t on every point set of the GPU
suite, and host.vecchia_order -- the same rule behind a k-d tree that proposes candidates -- returns the greedy's bits."""
import numpy as np
import pytest

import order_reference as OR

SETS = list(OR.point_sets()) + ["uniform 20000"]


@pytest.mark.parametrize("n", OR.LABEL_SIZES)
def test_labels_are_a_permutation(n):
    from cocons_amd import host
    lab = OR.labels(n)
    assert np.array_equal(np.sort(lab), np.arange(n))
    assert np.array_equal(OR.labels_fast(n), lab)
    assert np.array_equal(host._order_labels(n), lab)


@pytest.mark.parametrize("name", SETS)
def test_greedy_is_a_permutation_with_the_property(name):
    locs, order, counts = OR.reference(name)
    worst = OR.check_property(locs, order, counts)
    print("%s: n = %d, counts = %s, largest M_t / m_t = %.4f" % (name, locs.shape[0], counts.tolist(), worst))
    assert worst < 4.0


@pytest.mark.parametrize("name", SETS)
def test_host_order_equals_the_greedy(name):
    from cocons_amd import host
    locs, order, counts = OR.reference(name)
    got, got_counts = host.vecchia_order(locs, levels=True)
    assert got.dtype == np.int32 and np.array_equal(got, order)
    assert np.array_equal(got_counts, counts)
    assert np.array_equal(host.vecchia_order(locs), order)


def test_the_level_structure_is_the_rules():
    # a hand-checkable set: four corners of the unit square and its centre; L = 1, the centre is level 0, every corner is
    # sqrt(1/2) from it: d2 = 0.5 conflicts at level 1 (e = 1), not at level 2 (e = 0.25), where the corners (1 apart) all fit
    locs = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 0.5], [0.0, 1.0], [1.0, 1.0]])
    order, counts = OR.greedy(locs)
    assert order[0] == 3 and counts.tolist() == [1, 0, 4, 0]
    lab = OR.labels(5)
    corners = [i for i in np.argsort(lab) if i != 2]
    assert (order[1:] - 1).tolist() == corners
