"""The block form of the grouped Vecchia gradient (tests/vecchia_group_grad_reference.py) against the
per-observation statement (tests/vecchia_grad_reference.py) on the expanded table -- the same model -- without a GPU: value,
parts, the 6 x p table, the quadratic forms' share and the mean gradient agree within GRAD_TOL = 1e-7 of
tests/test_gpu_vecchia_grad.py, relative to the largest magnitude."""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import vecchia_grad_reference as VG  # noqa: E402
import vecchia_group_grad_reference as VGG  # noqa: E402
import vecchia_reference as VR  # noqa: E402

GRAD_TOL = 1e-7


@functools.lru_cache(maxsize=None)
def small_problem(n):
    """(locs, X, theta, z) in the shape of test_gpu_dense_sizes.problem, without the oracle's Sigma"""
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(6400 + n)
    p = 1 if n < 3 else 3
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n)] + [rng.standard_normal(n) * 0.5 for _ in range(p - 1)]))
    th = OrderedDict((k, np.array(v[:p], dtype=float)) for k, v in wl.theta_full(scale0=np.log(0.2)).items())
    th["mean"] = np.array([0.3, -0.15, 0.2])[:p]
    z = np.asfortranarray(rng.standard_normal((n, 2)))
    return locs, X, th, z


def _rel(got, want, scale=None):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want if scale is None else scale))), 1e-300))


def compare(n, nn, group, B=None):
    """the worst relative deviation of the block form from the per-observation statement on the expanded table"""
    from cocons_amd import host, workloads as wl
    locs, X, th, z = small_problem(n)
    T = host.theta_table(th)
    wide = GR.table(nn, group)
    assert GR.closed(wide, group) == 0
    want = VG.neg2loglik_grad(T, th["mean"], locs, X, z, wl.SMOOTH_LIMITS, wide, B=B)
    got = VGG.neg2loglik_grad(T, th["mean"], locs, X, z, wl.SMOOTH_LIMITS, wide, group, B=B)
    errs = [abs(got[0] - want[0]) / abs(want[0]), _rel(got[1], want[1]), _rel(got[2], want[2]), _rel(got[3], want[3], want[2])]
    if B is None:
        errs.append(_rel(got[4], want[4]))
    else:
        assert got[4] is None
    # the plan of the caller's table and of the expanded one are the same blocks
    assert GR.plan(nn, group)["mask"] == GR.plan(wide, group)["mask"]
    return max(errs)


@pytest.mark.parametrize("cap", (2, 17, 64))
@pytest.mark.parametrize("m", (1, 10))
@pytest.mark.parametrize("n", (2, 65, 300))
def test_greedy_groups(n, m, cap):
    from cocons_amd import host
    nn = host.vecchia_neighbours(small_problem(n)[0], m)
    err = compare(n, nn, GR.greedy(nn, cap))
    print("vecchia-group-grad-report cpu | block form against the per-observation statement | n%d m%d cap%d | %.2e" % (n, m, cap, err))
    assert err < GRAD_TOL


def test_interleaved_members_and_a_member_at_position_0():
    """rows in strides of 7: members with rows between them that are not, row 1 of the data a member of a larger block"""
    from cocons_amd import host
    n = 300
    nn = host.vecchia_neighbours(small_problem(n)[0], 4)
    stride = (np.arange(n) % 7 + 7 * (np.arange(n) // 49)).astype(np.int32)
    pl = GR.plan(nn, stride)
    first = pl["block"][0]
    assert pl["pos"][0] == 0 and pl["off"][first + 1] - pl["off"][first] > 1 and pl["mask"][first] & 1
    assert any((m >> q) & 7 == 5 for m in pl["mask"] for q in range(62))
    err = compare(n, nn, stride)
    print("vecchia-group-grad-report cpu | interleaved members, a member at position 0 | n%d blocks%d | %.2e" % (n, pl["blocks"], err))
    assert err < GRAD_TOL


def test_one_block_of_64_members_and_given_columns():
    n = 65
    locs = small_problem(n)[0]
    nn = np.zeros((n, 63), dtype=np.int32, order="F")
    nn[:64] = VR.all_predecessors(64)
    nn[64, :3] = (1, 2, 3)
    group = np.zeros(n, dtype=np.int32)
    group[64] = 1
    pl = GR.plan(nn, group)
    assert pl["mask"][0] == (1 << 64) - 1 and pl["maxrows"] == 64
    B = np.random.default_rng(5).standard_normal((n, 5))
    errs = (compare(n, nn, group), compare(n, nn, group, B=B))
    print("vecchia-group-grad-report cpu | one block of 64 members; five given columns | n%d | %.2e" % (n, max(errs)))
    assert locs.shape == (n, 2) and max(errs) < GRAD_TOL
