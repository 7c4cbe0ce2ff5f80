"""The block form of the grouped Vecchia information (tests/vecchia_group_fisher_reference.py) against the
per-observation statement (tests/vecchia_fisher_reference.py) on the expanded table -- the same model -- without a GPU: info
within 1e-12 in fisher_reference.metric, the bound the two numpy statements of the ungrouped entry hold each other to, and
info_mean within 1e-10 of its largest entry (test_vecchia_fisher_reference's bound for it)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
import group_reference as GR  # noqa: E402
import vecchia_fisher_reference as VF  # noqa: E402
import vecchia_group_fisher_reference as VGF  # noqa: E402
import vecchia_reference as VR  # noqa: E402

TOL = 1e-12
MEAN_TOL = 1e-10


def dirs_for(p):
    """the 6 p unit tables, then the scaling direction"""
    return np.concatenate([np.eye(6 * p).reshape(6 * p, 6, p), FR.scaling_direction(p)[None]])


@functools.lru_cache(maxsize=None)
def matrices(n):
    """(locs, X, Sigma, Sigma_a) of vecchia_fisher_reference.setup, p = 1 below three sites"""
    from cocons_amd import host, workloads as wl
    p = 1 if n < 3 else 3
    locs, X, th = VF.setup(n, p=p)
    S, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, dirs_for(p))
    S.setflags(write=False)
    Sa.setflags(write=False)
    return locs, X, S, Sa


def compare(n, nn, group, r=1):
    """(metric of info, relative deviation of info_mean) of the block form from the per-observation statement on the expanded
    table, and the block form's matrices"""
    locs, X, S, Sa = matrices(n)
    wide = GR.table(nn, group)
    assert GR.closed(wide, group) == 0
    want, wm = VF.info_last_row(S, Sa, wide, r, X)
    got, gm = VGF.info_blocks(S, Sa, GR.plan(wide, group), r, X)
    # the plan of the caller's table and of the expanded one are the same blocks
    assert GR.plan(nn, group)["mask"] == GR.plan(wide, group)["mask"]
    return FR.metric(got, want), float(np.max(np.abs(gm - wm)) / np.max(np.abs(wm))), got, gm


@pytest.mark.parametrize("cap", (2, 17, 64))
@pytest.mark.parametrize("m", (1, 10))
@pytest.mark.parametrize("n", (2, 65, 300))
def test_greedy_groups(n, m, cap):
    from cocons_amd import host
    nn = host.vecchia_neighbours(matrices(n)[0], m)
    err, em, info, _ = compare(n, nn, GR.greedy(nn, cap), r=2)
    print("vecchia-group-fisher-report cpu | block form against the per-observation statement (metric, mean) | n%d m%d cap%d | "
          "%.2e %.2e" % (n, m, cap, err, em))
    assert err <= TOL and em <= MEAN_TOL
    ev = np.linalg.eigvalsh(info)
    assert ev[0] >= -1e-12 * ev[-1]                      # positive semi-definite
    assert abs(info[-1, -1] - 2 * n / 2) <= 1e-12 * 2 * n    # the scaling direction: r n / 2


def test_interleaved_members_and_a_member_at_position_0():
    """rows in strides of 7: members with rows between them that are not, row 1 of the data a member of a larger block"""
    from cocons_amd import host
    n = 300
    nn = host.vecchia_neighbours(matrices(n)[0], 4)
    stride = (np.arange(n) % 7 + 7 * (np.arange(n) // 49)).astype(np.int32)
    pl = GR.plan(nn, stride)
    first = pl["block"][0]
    assert pl["pos"][0] == 0 and pl["off"][first + 1] - pl["off"][first] > 1 and pl["mask"][first] & 1
    assert any((m >> q) & 7 == 5 for m in pl["mask"] for q in range(62))
    err, em, _, _ = compare(n, nn, stride)
    print("vecchia-group-fisher-report cpu | interleaved members, a member at position 0 (metric, mean) | n%d blocks%d | %.2e %.2e"
          % (n, pl["blocks"], err, em))
    assert err <= TOL and em <= MEAN_TOL


def test_blocks_of_one_row():
    """every row its own block at m = 1: rows without a neighbour are blocks of one row, the others of two"""
    from cocons_amd import host
    n = 65
    nn = host.vecchia_neighbours(matrices(n)[0], 1).copy(order="F")
    nn[::3, 0] = 0
    group = np.arange(n, dtype=np.int32)
    pl = GR.plan(nn, group)
    assert pl["blocks"] == n and min(pl["off"][b + 1] - pl["off"][b] for b in range(n)) == 1
    err, em, _, _ = compare(n, nn, group)
    print("vecchia-group-fisher-report cpu | blocks of one and two rows (metric, mean) | n%d | %.2e %.2e" % (n, err, em))
    assert err <= TOL and em <= MEAN_TOL


def test_one_block_of_64_members_is_the_dense_information():
    n = 64
    locs, X, S, Sa = matrices(n)
    nn = VR.all_predecessors(n)
    group = np.zeros(n, dtype=np.int32)
    pl = GR.plan(nn, group)
    assert pl["blocks"] == 1 and pl["mask"][0] == (1 << 64) - 1 and pl["maxrows"] == 64
    got, gm = VGF.info_blocks(S, Sa, pl, 1, X)
    want = FR.info_solve(S, Sa, 1)
    err, em, _, _ = compare(n, nn, group)
    print("vecchia-group-fisher-report cpu | one block of 64 members vs FR.info_solve; vs the per-observation statement (metric) | "
          "n64 | %.2e %.2e" % (FR.metric(got, want), err))
    assert FR.metric(got, want) <= TOL and err <= TOL and em <= MEAN_TOL
    wm = X.T @ np.linalg.solve(S, X)                     # r (UX)'(UX) with U'U = Sigma^-1
    assert np.max(np.abs(gm - wm)) <= MEAN_TOL * np.max(np.abs(wm))


@pytest.mark.parametrize("r", (1, 3))
def test_info_mean_is_r_times_the_gram_of_UX(r):
    """U: row i holds s of observation i on the expanded table (the whitening); info_mean = r (UX)'(UX)"""
    from cocons_amd import host
    n = 150
    locs, X, S, Sa = matrices(n)
    nn = host.vecchia_neighbours(locs, 10)
    group = GR.greedy(nn, 17)
    wide = GR.table(nn, group)
    U = np.zeros((n, n))
    for i in range(n):
        idx = np.append(VR.rows_of(wide, i), i)
        e = np.zeros(idx.size)
        e[-1] = 1.0
        U[i, idx] = np.linalg.solve(np.linalg.cholesky(S[np.ix_(idx, idx)]).T, e)
    _, gm = VGF.info_blocks(S, Sa, GR.plan(nn, group), r, X)
    want = r * (U @ X).T @ (U @ X)
    assert np.max(np.abs(gm - want)) <= MEAN_TOL * np.max(np.abs(want))
