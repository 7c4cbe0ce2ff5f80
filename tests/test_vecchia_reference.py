"""The Vecchia reference (tests/vecchia_reference.py) and the host's neighbour search, without a GPU: the search equals brute
force; with every predecessor as a neighbour the reference is the exact dense value; with m = 10 .. 63 it is far enough from
the exact value (at least 1e-3 relative) that nothing which ignores the table can pass the GPU comparisons; and the double
reference sits within 1e-12 of its long-double twin.  The problem is test_gpu_dense_sizes.problem's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402


def _brute(locs, m):
    n = locs.shape[0]
    nn = np.zeros((n, m), dtype=np.int32)
    for i in range(1, n):
        d = np.hypot(locs[:i, 0] - locs[i, 0], locs[:i, 1] - locs[i, 1])
        o = np.lexsort((np.arange(i), d))[:m]
        nn[i, :o.size] = o + 1
    return nn


@pytest.mark.parametrize("m", (1, 10, 30))
def test_neighbour_search_equals_brute_force(m):
    from cocons_amd import host
    locs = np.array(problem(300)[0])
    locs[50] = locs[10]                 # coincident sites: row 200 sees rows 10 and 50 at distance 0, broken by index
    locs[200] = locs[10]
    locs[40] = [0.5078125, 0.5]         # an exact tie: rows 40 and 41 at distance 2^-7 of row 121
    locs[41] = [0.4921875, 0.5]
    locs[121] = [0.5, 0.5]
    nn = host.vecchia_neighbours(locs, m)
    assert nn.dtype == np.int32 and nn.flags.f_contiguous and nn.shape == (300, m)
    assert np.array_equal(nn, _brute(locs, m))
    for i in range(300):                # earlier rows only; short rows zero-padded behind their entries
        assert np.all(nn[i] < i + 1) and np.count_nonzero(nn[i]) == min(i, m)
    nnp = host.vecchia_neighbours_pred(locs, locs[:5] + 1e-3, m)
    for i in range(5):
        d = np.hypot(locs[:, 0] - locs[i, 0] - 1e-3, locs[:, 1] - locs[i, 1] - 1e-3)
        assert set(nnp[i] - 1) == set(np.argsort(d, kind="stable")[:m])


def test_all_predecessors_is_the_exact_value():
    locs, X, th, z, lp, Xp, S, Rz = problem(65)
    val, parts = VR.neg2loglik(S, VR.all_predecessors(65), Rz)
    exact = VR.neg2loglik_exact(S, Rz)
    rel = abs(val - exact) / abs(exact)
    print("vecchia-report reference | exact n65 m64 | rel %.2e" % rel)
    assert rel < 1e-12
    assert abs(parts[0] - np.sum(np.log(np.diag(np.linalg.cholesky(S))))) < 1e-10


@pytest.mark.parametrize("n,m", ((300, 10), (300, 30), (641, 30), (641, 63)))
def test_truncated_tables_differ_from_the_exact_value(n, m):
    from cocons_amd import host
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    nn = host.vecchia_neighbours(locs, m)
    val, _ = VR.neg2loglik(S, nn, Rz)
    exact = VR.neg2loglik_exact(S, Rz)
    gap = abs(val - exact) / abs(exact)
    print("vecchia-report reference | gap n%d m%d | rel %.2e" % (n, m, gap))
    assert gap >= 1e-3


def test_double_reference_against_long_double():
    from cocons_amd import host
    locs, X, th, z, lp, Xp, S, Rz = problem(300)
    nn = host.vecchia_neighbours(locs, 30)
    Y, logd = VR.whiten(S, nn, Rz)
    Yl, logdl = VR.whiten(S, nn, Rz, long_double=True)
    e = max(float(np.max(np.abs(Y - Yl))) / float(np.max(np.abs(Yl))), float(np.max(np.abs(logd - logdl))))
    dmin = float(np.exp(2 * np.min(logd)))
    print("vecchia-report reference | double vs long double n300 m30 | %.2e | smallest conditional variance %.3g" % (e, dmin))
    assert e < 1e-12 and dmin > 0
