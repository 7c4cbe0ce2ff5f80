"""The grouped Vecchia coefficients restated block by block (tests/vecchia_group_coef_reference.py) against the
per-observation statement tests/vecchia_sim_reference.coefficients on the expanded table, without a GPU.

The two are the same numbers in another summation order (numpy's blocked Cholesky of the whole block against one of every
leading sub-block), so the bound is set against a referee, not against each other: per case the block form's largest
row-relative error against coefficients(..., dtype=np.longdouble) may be at most 4 x the float64 per-observation statement's
own error against it, with a floor of 8 eps -- the 4 covers case-to-case scatter between two roundings of the same length.
The matrix is Matern-3/2 with a nugget on uniform sites.  Every test prints its ratio on a line that starts with
`vecchia-group-coef-report`; tests/golden/VECCHIA_GROUP_COEF_REPORT.md records them."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import vecchia_group_coef_reference as GC  # noqa: E402
import vecchia_sim_reference as SR  # noqa: E402

EPS = np.finfo(np.float64).eps
FACTOR, FLOOR = 4.0, 8.0 * EPS


@functools.lru_cache(maxsize=None)
def _sites(n):
    locs = np.random.default_rng(4100 + n).uniform(size=(n, 2))
    locs.setflags(write=False)
    return locs


@functools.lru_cache(maxsize=None)
def _matrix(n, rho):
    locs = _sites(n)
    d = np.sqrt(3.0) * np.hypot(locs[:, None, 0] - locs[None, :, 0], locs[:, None, 1] - locs[None, :, 1]) / rho
    S = (1.0 + d) * np.exp(-d) + 0.05 * np.eye(n)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _tables(n, m, cap):
    from cocons_amd import host
    nn = host.vecchia_neighbours(_sites(n), m)
    group = GR.greedy(nn, cap)
    wide = GR.table(nn, group)
    for a in (nn, group, wide):
        a.setflags(write=False)
    return nn, group, wide


@functools.lru_cache(maxsize=None)
def _referee(n, m, cap, rho):
    """(long double coefficients on the expanded table, the float64 per-observation statement)"""
    wide = _tables(n, m, cap)[2]
    S = _matrix(n, rho)
    return SR.coefficients(S, wide, dtype=np.longdouble), SR.coefficients(S, wide)


def _row_rel(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    scale = np.max(np.abs(want), axis=1)
    return float(np.max(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want), axis=1) / scale))


CASES = ((65, 10, 17, 0.3), (300, 30, 64, 0.3), (300, 30, 64, 0.05), (300, 10, 2, 0.3))


@pytest.mark.parametrize("n,m,cap,rho", CASES)
def test_block_form_against_the_long_double_referee(n, m, cap, rho):
    nn, group, wide = _tables(n, m, cap)
    ref, plain = _referee(n, m, cap, rho)
    got = GC.coefficients(_matrix(n, rho), wide, group)
    own, err = _row_rel(plain, ref), _row_rel(got, ref)
    bound = max(FACTOR * own, FLOOR)
    print("vecchia-group-coef-report cpu | block form against the long double referee (error, statement's own, ratio) | "
          "n%d m%d cap%d rho%.2f | %.2e %.2e %.2f" % (n, m, cap, rho, err, own, err / own))
    assert err <= bound, (err, own)
    # the zeros stand in the places p .. m - 1
    pl = GR.plan(wide, group)
    mw = wide.shape[1]
    for i in range(n):
        assert np.all(got[i, pl["pos"][i]:mw] == 0.0) and got[i, mw] > 0.0


def test_n_fixed_writes_the_later_rows_only():
    n, m, cap, rho = 300, 30, 64, 0.3
    nn, group, wide = _tables(n, m, cap)
    S = _matrix(n, rho)
    full = GC.coefficients(S, wide, group)
    pl = GR.plan(wide, group)
    # a row in the middle of a block with members on both sides, the last row, a row past the whole first blocks
    big = max(range(pl["blocks"]), key=lambda b: bin(pl["mask"][b]).count("1"))
    mem = [int(r) for q, r in enumerate(pl["rows"][pl["off"][big]:pl["off"][big + 1]]) if (pl["mask"][big] >> q) & 1]
    assert len(mem) >= 3
    for nf in (mem[len(mem) // 2], n - 1, int(np.max(pl["rows"][:pl["off"][3]])) + 1):
        part = GC.coefficients(S, wide, group, n_fixed=nf, fill=np.nan)
        assert np.all(np.isnan(part[:nf])) and np.array_equal(part[nf:], full[nf:])
        print("vecchia-group-coef-report cpu | n_fixed writes the rows behind it alone | n%d n_fixed%d | 0" % (n, nf))


def test_a_table_padded_wider_than_its_longest_row():
    n, m, cap, rho = 65, 10, 17, 0.3
    nn, group, wide = _tables(n, m, cap)
    S = _matrix(n, rho)
    got = GC.coefficients(S, wide, group)
    padded = GR.table(nn, group, m_out=63)
    assert padded.shape[1] == 63 and wide.shape[1] < 63 and GR.closed(padded, group) == 0
    wider = GC.coefficients(S, padded, group)
    mw = wide.shape[1]
    assert wider.shape == (n, 64)
    assert np.array_equal(wider[:, :mw], got[:, :mw]) and np.array_equal(wider[:, 63], got[:, mw])
    assert np.all(wider[:, mw:63] == 0.0)
    assert np.array_equal(GC.coefficients(S, wide, group, m_out=63), wider)
    print("vecchia-group-coef-report cpu | the same numbers at the stride of a table padded to m = 63 | n%d | 0" % n)
