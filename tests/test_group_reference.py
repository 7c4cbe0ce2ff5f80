"""What grouping does to the model, on the CPU: tests/group_reference.py's rule and expanded table under
tests/vecchia_reference.py on the oracle's Sigma, and the library's host entries (cocons_vecchia_group,
cocons_vecchia_group_table -- plain host code, no device) against the restatement."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402


@functools.lru_cache(maxsize=None)
def tables(n, m, max_rows=64):
    """(the m nearest earlier observations, the greedy groups, the expanded table) on problem(n)'s sites"""
    from cocons_amd import host
    nn = host.vecchia_neighbours(problem(n)[0], m)
    group = GR.greedy(nn, max_rows)
    wide = GR.table(nn, group)
    for a in (nn, group, wide):
        a.setflags(write=False)
    return nn, group, wide


def test_the_expanded_table_changes_the_value():
    """nothing that ignores the groups can pass for the grouped model: the two values differ by more than 1e-6 relative"""
    n, m = 300, 10
    S, Rz = problem(n)[6], problem(n)[7]
    nn, group, wide = tables(n, m)
    a, b = VR.neg2loglik(S, nn, Rz)[0], VR.neg2loglik(S, wide, Rz)[0]
    print("vecchia-group-report cpu | value on the input table %.10f, on the expanded table %.10f | n%d m%d | rel %.2e"
          % (a, b, n, m, abs(a - b) / abs(a)))
    assert abs(a - b) / abs(a) > 1e-6


def test_one_block_of_all_rows_is_the_dense_value():
    """n = 64, every predecessor a neighbour, one block: the expanded table is the input table and the value is exact"""
    n = 64
    S, Rz = problem(65)[6][:n, :n], problem(65)[7][:n]
    every = VR.all_predecessors(n)
    group = np.zeros(n, dtype=np.int32)
    wide = GR.table(every, group)
    assert np.array_equal(wide, every) and GR.closed(every, group) == 0
    pl = GR.plan(every, group)
    assert pl["blocks"] == 1 and pl["mask"] == [2 ** 64 - 1]
    got, exact = VR.neg2loglik(S, wide, Rz)[0], VR.neg2loglik_exact(S, Rz)
    assert abs(got - exact) / abs(exact) < 1e-11


def _kl(S, nn):
    """KL(N(0, Sigma) || N(0, (U'U)^-1)) = (tr(U'U Sigma) - n + log|(U'U)^-1| - log|Sigma|) / 2"""
    Q = VR.precision_matrix(S, nn)[0]
    logd = VR.whiten(S, nn, np.zeros((S.shape[0], 1)))[1]
    return 0.5 * float(np.trace(Q @ S) - S.shape[0] + 2 * np.sum(logd) - np.linalg.slogdet(S)[1])


@pytest.mark.parametrize("m", (5, 10))
def test_grouping_never_raises_the_kl_divergence(m):
    """every member conditions on a superset of its neighbours, and a larger conditioning set never raises the KL divergence
    from the exact model: a theorem, not a measured margin (the Bessel branch, theta_full)"""
    n = 300
    S = problem(n)[6]
    nn, group, wide = tables(n, m)
    plain, grouped = _kl(S, nn), _kl(S, wide)
    print("vecchia-group-report cpu | KL ungrouped %.6e grouped %.6e | n%d m%d" % (plain, grouped, n, m))
    assert grouped <= plain


@pytest.mark.parametrize("n,m,max_rows", ((1, 1, 2), (65, 10, 17), (300, 10, 64), (641, 30, 64)))
def test_library_entries_equal_the_restatement(n, m, max_rows):
    import cocons_amd as ca
    nn = tables(n, m, max_rows)[0]
    group, st = ca.vecchia_group(nn, max_rows, stats=True)
    want = GR.greedy(nn, max_rows)
    pl = GR.plan(nn, want)
    assert np.array_equal(group, want)
    assert st == {"blocks": pl["blocks"], "rows": pl["sum_rows"], "pairs": pl["pairs"], "pairs_ungrouped": GR.pairs_ungrouped(nn)}
    assert np.array_equal(ca.vecchia_group_table(nn, group), GR.table(nn, want))
    assert np.array_equal(ca.vecchia_group_table(nn, group, 63), GR.table(nn, want, 63))
    # any partition, labels in any numbering
    other = (np.arange(n)[::-1] // 2).astype(np.int32)
    try:
        wide = GR.table(nn, other)
    except ValueError:
        wide = None
    if wide is not None:
        assert np.array_equal(ca.vecchia_group_table(nn, other), wide)


def test_plan_statistics_of_a_uniform_design():
    """cocons_vecchia_group's out4 at n = 641, m = 30 on uniform sites: the grouped schedule evaluates fewer pairs"""
    import cocons_amd as ca
    st = ca.vecchia_group(tables(641, 30)[0], 64, stats=True)[1]
    print("vecchia-group-report cpu | plan statistics n641 m30 | %s" % st)
    assert st["pairs"] < st["pairs_ungrouped"]


def test_host_entries_refuse_with_their_names():
    import cocons_amd as ca
    from cocons_amd import _lib
    nn = np.array(tables(65, 10)[0], order="F")

    def refused(call, *words):
        with pytest.raises(_lib.CoconsHipError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: ca.vecchia_group(nn, 1), "cocons_vecchia_group:", "max_rows = 1")
    refused(lambda: ca.vecchia_group(nn, 65), "cocons_vecchia_group:", "max_rows = 65")
    late = nn.copy(order="F")
    late[5, 0] = 6
    refused(lambda: ca.vecchia_group(late, 64), "cocons_vecchia_group:", "row 6 ")
    twice = nn.copy(order="F")
    twice[10, 0] = twice[10, 1] = 3
    refused(lambda: ca.vecchia_group_table(twice, np.zeros(65, dtype=np.int32)), "cocons_vecchia_group_table:", "row 11 ", "twice")
    refused(lambda: ca.vecchia_group_table(nn, np.zeros(65, dtype=np.int32)), "cocons_vecchia_group_table:", "block of row 1 ",
            "more than 64 rows")
    group = ca.vecchia_group(nn, 64)
    refused(lambda: ca.vecchia_group_table(nn, group, 1), "cocons_vecchia_group_table:", "m_out = 1", "longest expanded row")
    refused(lambda: ca.vecchia_group_table(nn, group, 64), "cocons_vecchia_group_table:", "m_out = 64")
    bad = group.copy()
    bad[7] = 65
    refused(lambda: ca.vecchia_group_table(nn, bad), "cocons_vecchia_group_table:", "group[7]")
