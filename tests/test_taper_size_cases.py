"""tests/taper_size_cases.py (the sizes of tests/test_gpu_taper_sizes.py) on the CPU: every size shows the row of the table
it claims, in the library's order and in the caller's; the matrices are conditioned like those the suite's tolerances were
set at; the prediction sets hold the rows they promise; the references the GPU tests lean on run at every size, n = 1
included, and say there what they must; and the library's own envelope rule (cocons_amd/csrc/band_plan.hpp, compiled into
tests/band_plan_main.cpp by the host compiler) gives the table integer for integer where its floor is clipped (nt <= 4) and
where the last block of two tile columns holds one.  No GPU."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_reference as CV  # noqa: E402
import grad_taper_reference as GT  # noqa: E402
import taper_envelope_cases as TE  # noqa: E402
import taper_size_cases as TS  # noqa: E402
from test_taper_envelope_cases import _pattern_in_order, _prefix, _run_band_plan, band_plan_exe  # noqa: E402,F401

COND_CAP = 2000.0
ORDERS = [(n, True) for n in TS.TAPER_SIZES] + [(n, False) for n in TS.CALLER_ORDER_SIZES]


@functools.lru_cache(maxsize=None)
def _matrix(n):
    from cocons_amd.host import theta_table
    p = TS.problem(n)
    S, _ = GT.taper_matrix(theta_table(p.theta), p.locs, p.X, TE.SMOOTH_LIMITS, p.ref_taper)
    S = np.tril(S) + np.tril(S, -1).T
    S.setflags(write=False)
    return S


def test_the_sizes_are_the_issue():
    assert TS.TAPER_SIZES == (1, 2, 63, 64, 65, 127, 128, 129, 192, 256, 257, 384, 512, 640)
    assert sorted(TS.TABLE) == sorted(TS.TAPER_SIZES)
    assert sorted({TS.TABLE[n][0] for n in TS.TAPER_SIZES}) == [1, 2, 3, 4, 5]          # nt = 1 ... 5
    assert [n for n in TS.TAPER_SIZES if TS.TABLE[n][2]] == [640]                        # the one packed case
    assert [n for n in TS.TAPER_SIZES if n % TE.TILE == 0] == [128, 256, 384, 512, 640]  # no ragged tile
    assert TS.M_PRED == 130 and len({TS.ON_TOP // 64, TS.EMPTY // 64}) == 2 and TS.EMPTY // 64 == 2


@pytest.mark.parametrize("n", TS.TAPER_SIZES)
def test_table_in_both_orders(n):
    p = TS.problem(n)
    ci, rp, _ = p.ref_taper
    order = TS.order_of(p)
    assert sorted(order.tolist()) == list(range(1, n + 1))
    nt, hi, W, packed = TE.envelope_of(n, ci, rp, order)
    print("n %d: nt %d W %d packed %s hi %s" % (n, nt, W, packed, hi.tolist()))
    TS.assert_shape(n, nt, hi, W, packed)
    if n == 640:                  # the floor alone: the pattern asks for less
        assert np.array_equal(hi, TE.floor_envelope(nt))
        assert np.all(TE.raw_skyline(n, ci, rp, order)[1] <= hi)
    caller = TS.problem(n, rcm=False)
    assert not caller.rcm and caller.locs is p.locs
    ident = TS.order_of(caller)
    assert np.array_equal(ident, np.arange(1, n + 1))
    nt, hi, W, packed = TE.envelope_of(n, ci, rp, ident)
    TS.assert_shape(n, nt, hi, W, packed, rcm=False)


@pytest.mark.parametrize("n", TS.TAPER_SIZES)
def test_problem_is_what_it_claims(n):
    p = TS.problem(n)
    cols = TS.columns_of(n)
    assert cols == (1 if n < 3 else 3)
    assert p.n == n and p.locs.shape == (n, 2) and p.X.shape == (n, cols) and p.z.shape == (n, 2)
    assert np.all(p.X[:, 0] == 1.0) and np.all((p.locs >= 0) & (p.locs <= 1))
    assert p.delta == (0.25 if n <= 384 else 0.15)
    want = TE.theta_full()
    assert list(p.theta) == list(want) and all(np.array_equal(p.theta[k], want[k][:cols]) for k in want)
    if n >= 3:
        assert np.linalg.matrix_rank(p.X) == 3
    # the pattern: 1-based CSR, symmetric, diagonal stored with taper 1, columns ascending, no stored zero
    ci, rp, ent = p.ref_taper
    rows = np.repeat(np.arange(n), np.diff(rp))
    A = np.full((n, n), -1.0)
    A[rows, ci - 1] = ent
    assert rp[0] == 1 and rp[-1] == ci.size + 1 and np.array_equal(A, A.T)
    assert np.all(np.diag(A) == 1.0) and np.all(ent > 0) and np.all(ent <= 1)
    assert all(np.all(np.diff(ci[rp[i] - 1:rp[i + 1] - 1]) > 0) for i in range(n))
    S = _matrix(n)
    cond = float(np.linalg.cond(S))
    print("n %d: cond(S) %.3g, %d stored entries" % (n, cond, ci.size))
    assert cond <= COND_CAP, cond
    assert np.all(np.isfinite(S)) and np.array_equal(S, S.T)


@pytest.mark.parametrize("n", TS.TAPER_SIZES)
def test_prediction_set(n):
    p = TS.problem(n)
    ci, rp, ent = p.pred_taper
    _, empty, on_top = p.special
    assert (empty, on_top) == (TS.EMPTY, TS.ON_TOP)
    assert p.lp.shape == (TS.M_PRED, 2) and p.Xp.shape == (TS.M_PRED, TS.columns_of(n))
    assert rp.size == TS.M_PRED + 1 and rp[0] == 1 and rp[-1] == ci.size + 1
    cnt = np.diff(rp)
    assert cnt[empty] == 0 and np.array_equal(p.lp[empty], [4.0, 4.0])
    assert np.array_equal(p.lp[on_top], p.locs[(3 * n) // 7])
    mine = slice(rp[on_top] - 1, rp[on_top + 1] - 1)
    assert (3 * n) // 7 + 1 in ci[mine] and ent[mine][ci[mine] == (3 * n) // 7 + 1] == 1.0
    assert all(np.all(np.diff(ci[rp[i] - 1:rp[i + 1] - 1]) > 0) for i in range(TS.M_PRED))
    others = np.delete(np.arange(TS.M_PRED), [empty, on_top])
    assert np.all((p.lp[others] >= 0) & (p.lp[others] <= 1))
    # the pattern among the prediction rows: every row holds its diagonal, the row without a neighbour nothing else
    cu, ru, tu = TS.uu_pattern(n)
    for i in range(TS.M_PRED):
        w = slice(ru[i] - 1, ru[i + 1] - 1)
        assert i + 1 in cu[w] and np.all(np.diff(cu[w]) > 0)
    assert ru[empty + 1] - ru[empty] == 1
    one = TS.sub_pattern((cu, ru, tu), np.arange(1))
    assert one[0].tolist() == [1] and one[1].tolist() == [1, 2] and one[2].tolist() == [1.0]
    rows = TS.draw_rows()
    assert rows.size == TS.M_PRED - 1 and on_top not in rows and empty in rows and rows[0] == 0
    sub = TS.sub_pattern((cu, ru, tu), rows)
    D = np.zeros((TS.M_PRED, TS.M_PRED))
    D[np.repeat(np.arange(TS.M_PRED), np.diff(ru)), cu - 1] = tu
    D2 = np.zeros((rows.size, rows.size))
    D2[np.repeat(np.arange(rows.size), np.diff(sub[1])), sub[0] - 1] = sub[2]
    assert np.array_equal(D2, D[np.ix_(rows, rows)]) and sub[1][-1] == sub[0].size + 1
    # a row other than the one on top of an observation has a neighbour: the stochastic part has a scale without it
    assert np.any(np.delete(cnt, on_top) > 0)
    # the rows 0, 0 ... 63 and 64 ... 129 the held-factor test asks for alone
    for idx in (np.arange(1), np.arange(64), np.arange(64, TS.M_PRED)):
        c2, r2, e2 = TS.take_rows(p.pred_taper, idx)
        assert r2[-1] == c2.size + 1 == e2.size + 1 and np.array_equal(np.diff(r2), cnt[idx])


@pytest.mark.parametrize("n", TS.TAPER_SIZES)
def test_references_run_at_every_size(n):
    """cv_brute against cv_kroute at every observation (1e-12; brute force is n Cholesky factors of order n - 1, cheap here),
    the gradient's and the information's statements; at n = 1 leaving the observation out leaves nothing: the error is the
    residual and the variance S_11."""
    import fisher_taper_reference as FT
    from cocons_amd.host import theta_table
    p = TS.problem(n)
    S = _matrix(n)
    R = p.z - (p.X @ p.theta["mean"])[:, None]
    eb, vb = CV.cv_brute(S, R, np.arange(n))
    ek, vk = CV.cv_kroute(S, R, np.arange(n))
    ge, gv = CV.gaps(ek, vk, eb, vb)
    print("n %d: the two leave-one-out references %.2e %.2e" % (n, ge, gv))
    assert ge <= 1e-12 and gv <= 1e-12
    if n == 1:
        assert np.array_equal(eb, R) and vb[0] == S[0, 0]
        assert np.allclose(ek, R, rtol=1e-15, atol=0) and np.isclose(vk[0], S[0, 0], rtol=1e-15, atol=0)
    cols = TS.columns_of(n)
    f, parts, gl, gq, gm = GT.neg2loglik_taper_grad(theta_table(p.theta), p.theta["mean"], p.locs, p.X, p.z, TE.SMOOTH_LIMITS,
                                                    p.ref_taper)
    assert np.isfinite(f) and parts.shape == (3,) and gl.shape == gq.shape == (6, cols) and gm.shape == (cols,)
    ident = (gl + gq)[0, 0] + (gl + gq)[5, 0] - (2 * n - float(np.sum(parts[1:])))       # the scaling identity
    assert abs(ident) <= 1e-9 * 2 * n
    dirs = FT.standard_directions(cols)
    S2, Sa = FT.direction_matrices(theta_table(p.theta), p.locs, p.X, TE.SMOOTH_LIMITS, p.ref_taper, dirs)
    I = FT.info_whiten(S2, Sa, 1)
    assert I.shape == (3 * cols + 2,) * 2 and np.all(np.isfinite(I))
    assert abs(I[-1, -1] - n / 2) <= 1e-10 * n                                            # I(v_s, v_s) = r n / 2


@pytest.mark.parametrize("n", TS.TAPER_SIZES)
def test_predictive_covariance_of_the_reference(oracle, n):
    """What the GPU test of the joint prediction leans on (its dense numpy statement, on the CPU oracle's entries): the
    predictive covariance of the rows a draw is asked for is positive definite; the predictive variance of the row on top of
    an observation is far from zero with p = 3 (either sign: sd.pred is the root of its absolute value, well conditioned) and
    zero to rounding with the intercept alone, where the stochastic part there is the observation's residual."""
    from test_gpu_taper_sizes import _ref_joint
    p = TS.problem(n)
    st, Su, cov, mu = _ref_joint(n)
    rows = TS.draw_rows()
    ev = np.linalg.eigvalsh(cov[np.ix_(rows, rows)])
    var = cov[TS.ON_TOP, TS.ON_TOP]
    print("n %d: eigenvalues on the draw rows %.3g .. %.3g, on all rows from %.3g; variance on top of the observation %.3g"
          % (n, ev[0], ev[-1], np.linalg.eigvalsh(cov)[0], var))
    assert ev[0] >= 0.01
    assert cov[TS.EMPTY, TS.EMPTY] == Su[TS.EMPTY, TS.EMPTY] and np.count_nonzero(cov[TS.EMPTY]) == 1 and st[TS.EMPTY] == 0.0
    if n >= 3:
        assert abs(var) >= 1e-3          # an error of 1e-13 in it is one of 1.6e-12 in its root
    else:
        assert abs(var) <= 1e-14 * Su[TS.ON_TOP, TS.ON_TOP]
        resid = p.z[0, 0] - p.X[0] @ p.theta["mean"]
        assert abs(st[TS.ON_TOP] - resid) <= 1e-14 * abs(resid)


# --------------------------------------------------------------------------- the library's rule itself (band_plan.hpp)
@pytest.mark.parametrize("n,rcm", ORDERS)
def test_library_rule_gives_the_table(n, rcm, band_plan_exe, tmp_path):
    """band_envelope where it degenerates: the floor min((c & ~1) + 4, nt) clipped by nt <= 4, the last block of two tile
    columns holding one (odd nt), W = nt unpacked by rule, and the first packed size; hib and both prefix tables with it."""
    p = TS.problem(n, rcm)
    order = TS.order_of(p)
    nt, hi, W, packed = TE.envelope_of(n, p.ref_taper[0], p.ref_taper[1], order)
    prp, pci = _pattern_in_order(p, order)
    got = _run_band_plan(band_plan_exe, tmp_path / "pattern.txt",
                         "%d\n%s\n%s\n" % (n, " ".join(map(str, prp.tolist())), " ".join(map(str, pci.tolist()))))
    hib = TE.mirrored_envelope(hi)
    cols = np.arange(nt)
    print("n %d rcm %s: hi %s hib %s W %s" % (n, rcm, got["hi"], got["hib"], got["W"]))
    assert got["status"] == [0]
    assert got["nt"] == [nt] and got["maxband"] == [W] and got["W"] == [W]
    assert got["envelope"] == hi.tolist() and got["hi"] == hi.tolist() and got["hib"] == hib.tolist()
    assert got["toff"] == _prefix(hi - cols) and got["toffb"] == _prefix(hib - cols)
    if rcm:
        assert (got["nt"][0], got["W"][0], got["hi"]) == (TS.TABLE[n][0], TS.TABLE[n][1], TS.TABLE[n][3])
    if n == 640 and rcm:
        assert got["hib"] == [3, 5, 5, 5, 5]          # tile row 4 starts in tile column 2: the flipped factor's first column is short
