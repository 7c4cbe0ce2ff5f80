"""Grouped Vecchia blocks on the GPU (cocons_vecchia_set_groups, cocons_fit_create_vecchia_grouped,
cocons_neg2loglik_vecchia_grouped, cocons_vecchia_whiten_grouped), on the problem of
test_gpu_dense_sizes.problem.

Two kinds of comparison.  BITS: the grouped entries against the ungrouped entries on the same handle -- value, parts, every
whitened value and every log d must be equal, no tolerance.  PARITY: the same outputs against tests/vecchia_reference.py on
the expanded table (tests/group_reference.py) within the project's bound PARITY = 1e-8 of test_gpu_dense_sizes, relative to the
largest magnitude of the compared array or to |value|.  Every test prints its worst deviation on one line that starts with
`vecchia-group-report`; the measured figures stand in tests/golden/VECCHIA_GROUP_REPORT.md."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import PARITY, problem  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 65, 300, 641)
MS = (1, 10, 30)
CAPS = (2, 17, 64)
COLS = (1, 4, 5, 9)


def _report(what, case, err):
    print("vecchia-group-report gpu | %s | %s | %.2e" % (what, case, err))


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


@functools.lru_cache(maxsize=None)
def tables(n, m, max_rows):
    """(the m nearest earlier observations, the greedy groups, the expanded table) by the restatement"""
    from cocons_amd import host
    nn = host.vecchia_neighbours(problem(n)[0], m)
    group = GR.greedy(nn, max_rows)
    wide = GR.table(nn, group)
    for a in (nn, group, wide):
        a.setflags(write=False)
    return nn, group, wide


@functools.lru_cache(maxsize=None)
def columns(n, c):
    B = np.asfortranarray(np.random.default_rng(8800 + n).standard_normal((n, 9))[:, :c])
    B.setflags(write=False)
    return B


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _bits(f, th, n, cols=COLS):
    """grouped against ungrouped on the handle f: value, parts, whitened columns and log d; returns the ungrouped outputs"""
    v0, p0 = f.neg2loglik_core(th)
    v1, p1 = f.neg2loglik_core(th, grouped=True)
    assert v1 == v0 and _same(p1, p0), (v1 - v0, p1 - p0)
    out = [v0, p0]
    for c in cols:
        Y0, l0 = f.whiten_core(th, columns(n, c))
        Y1, l1 = f.whiten_grouped_core(th, columns(n, c))
        assert _same(Y1, Y0) and _same(l1, l0), (c, float(np.max(np.abs(Y1 - Y0))), float(np.max(np.abs(l1 - l0))))
        out += [Y0, l0]
    return out


def _parity(f, th, S, wide, Rz, case):
    val, parts = VR.neg2loglik(S, wide, Rz)
    Y, logd = VR.whiten(S, wide, Rz)
    gv, gp = f.neg2loglik_core(th, grouped=True)
    gY, gl = f.whiten_grouped_core(th, Rz)
    errs = (abs(gv - val) / abs(val), _rel(gp, parts), _rel(gY, Y), _rel(gl, logd))
    _report("parity with the restatement on the expanded table", case, max(errs))
    assert max(errs) < PARITY, errs


def _grouped_fit(n, m, max_rows, smooth_limits=None):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = problem(n)[:4]
    return ca.CoconsVecchiaFit.from_groups(locs, X, z, smooth_limits or wl.SMOOTH_LIMITS, tables(n, m, max_rows)[0], max_rows)


@pytest.mark.parametrize("max_rows", CAPS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_bits_and_parity_on_the_greedy_groups(n, m, max_rows):
    """the Bessel branch (theta_full): blocks of 1 .. max_rows rows (single rows keep their m + 1), the 64 / 65 seam, 1, 4, 5
    and 9 columns -- a partial last group of four"""
    th, S, Rz = problem(n)[2], problem(n)[6], problem(n)[7]
    nn, group, wide = tables(n, m, max_rows)
    f = _grouped_fit(n, m, max_rows)
    try:
        assert f.m == wide.shape[1]
        info = f.groups_info()
        pl = GR.plan(wide, group)
        assert (info["blocks"], info["maxrows"], info["rows"], info["pairs"]) == (pl["blocks"], pl["maxrows"], pl["sum_rows"], pl["pairs"])
        _bits(f, th, n)
        _report("bits: value parts whitened logd, c in 1 4 5 9", "n%d m%d cap%d blocks%d" % (n, m, max_rows, info["blocks"]), 0.0)
        _parity(f, th, S, wide, Rz, "n%d m%d cap%d" % (n, m, max_rows))
    finally:
        f.close()


@pytest.mark.parametrize("nu", (0.5, 1.5, 2.5))
def test_closed_form_modes(nu):
    from oracle import oracle as O
    n, m, cap = 300, 30, 64
    locs, X, th0, z = problem(n)[:4]
    th = OrderedDict((k, np.array(v, copy=True)) for k, v in th0.items())
    th["smooth"] = np.zeros(3)
    S = O.cov_rns(th, locs, X, (nu, nu))
    Rz = z - (X @ th["mean"])[:, None]
    f = _grouped_fit(n, m, cap, smooth_limits=(nu, nu))
    try:
        _bits(f, th, n, cols=(5,))
        _report("bits: closed form", "nu%.1f n%d m%d cap%d" % (nu, n, m, cap), 0.0)
        _parity(f, th, S, tables(n, m, cap)[2], Rz, "nu%.1f n%d m%d cap%d" % (nu, n, m, cap))
    finally:
        f.close()


def _hand_fit(n, nn, group):
    """the handle of the expanded table of a hand-made partition, the plan attached; (fit, expanded table, restated plan)"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = problem(n)[:4]
    wide = ca.vecchia_group_table(nn, group)
    assert _same(wide, GR.table(nn, group))
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    f.set_groups(group)
    return f, wide, GR.plan(wide, group)


def test_one_block_of_64_member_rows_is_the_dense_value():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 64
    locs, X, th, z = (a[:n] if i != 2 else a for i, a in enumerate(problem(65)[:4]))
    S, Rz = problem(65)[6][:n, :n], problem(65)[7][:n]
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    try:
        info = f.set_groups(np.zeros(n, dtype=np.int32))
        assert (info["blocks"], info["maxrows"], info["pairs"]) == (1, 64, 2016)
        v0, p0 = f.neg2loglik_core(th)
        v1, p1 = f.neg2loglik_core(th, grouped=True)
        Y0, l0 = f.whiten_core(th, Rz)
        Y1, l1 = f.whiten_grouped_core(th, Rz)
        assert v1 == v0 and _same(p1, p0) and _same(Y1, Y0) and _same(l1, l0)
        exact = VR.neg2loglik_exact(S, Rz)
        _report("one block of 64 members against the exact dense value", "n64", abs(v1 - exact) / abs(exact))
        assert abs(v1 - exact) / abs(exact) < PARITY
    finally:
        f.close()


def test_hand_made_partitions():
    """a block of 64 rows with a single member; members interleaved with rows that are not; a member at position 0 inside a
    larger block; blocks of one row"""
    from cocons_amd import host
    n = 300
    th = problem(n)[2]
    locs = problem(n)[0]
    # row 200 names its 63 nearest predecessors and stands alone; every other row is a block of its own with 3 neighbours
    nn = np.zeros((n, 63), dtype=np.int32, order="F")
    nn[:, :3] = host.vecchia_neighbours(locs, 3)
    nn[199] = host.vecchia_neighbours(locs[:200], 63)[199]
    own = np.arange(n, dtype=np.int32)
    f, wide, pl = _hand_fit(n, nn, own)
    try:
        assert pl["maxrows"] == 64 and pl["mask"][199] == 1 << 63 and pl["mask"][0] == 1 and pl["blocks"] == n
        _bits(f, th, n, cols=(5,))
        _report("bits: 64 rows with one member, blocks of one row", "n%d" % n, 0.0)
    finally:
        f.close()
    # rows in strides of 7 from the first row on: members with rows between them that are not, row 1 of the data a member
    nn = host.vecchia_neighbours(locs, 4)
    stride = (np.arange(n) % 7 + 7 * (np.arange(n) // 49)).astype(np.int32)
    f, wide, pl = _hand_fit(n, nn, stride)
    try:
        first = pl["block"][0]
        size = pl["off"][first + 1] - pl["off"][first]
        assert pl["pos"][0] == 0 and size > 1 and pl["mask"][first] & 1
        assert any((m >> q) & 7 == 5 for m in pl["mask"] for q in range(62))       # member, not a member, member
        _bits(f, th, n, cols=(5,))
        _report("bits: interleaved members, a member at position 0", "n%d blocks%d maxrows%d" % (n, pl["blocks"], pl["maxrows"]), 0.0)
    finally:
        f.close()


def _raw_value(f, th, grouped):
    from cocons_amd import host
    val, parts = ctypes.c_double(123.0), np.full(1 + f.r, 7.0)
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    entry = f._L.cocons_neg2loglik_vecchia_grouped if grouped else f._L.cocons_neg2loglik_vecchia
    rc = entry(f._h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts))
    return rc, val.value, parts


def _failing_fit(same_covariates):
    """test_gpu_vecchia's failing case -- observation 58 on the coordinates of observation 41 and conditioned on it -- with
    the rows 58, 61 and 65 in one block: the pivot of row 58 fails with rows behind it in the block"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from test_gpu_vecchia import _duplicate_site
    locs, X, th0, z, nn = _duplicate_site(same_covariates)
    n = 65
    group = np.arange(n, dtype=np.int32)
    group[[60, 64]] = group[57]
    wide = ca.vecchia_group_table(nn, group)
    pl = GR.plan(wide, group)
    b = pl["block"][57]
    assert 0 < pl["pos"][57] < pl["off"][b + 1] - pl["off"][b] - 1 and 41 in wide[57] and pl["mask"][b] >> pl["pos"][57] != 1
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    f.set_groups(group)
    return f, X, th0, z


def test_failing_block_in_the_middle_of_a_group():
    """Every member from the failing pivot on fails -- the rows the ungrouped entry reports, the smallest of them first: the
    same return code and failure word, the outputs left alone, and the next call on the handle clean.  Identical covariates:
    the second pivot of the pair is exactly 0.  Different covariates: the sign of the std.dev slopes decides (see
    test_gpu_vecchia.test_a_good_theta_keeps_its_bits_after_failures)."""
    from cocons_amd import _lib
    from test_gpu_vecchia import _theta
    f, X, th0, z = _failing_fit(True)
    try:
        bad = _theta(th0, std_dev=np.zeros(3), nugget=[-np.inf, 0.0, 0.0])
        plain, grouped = _raw_value(f, bad, False), _raw_value(f, bad, True)
        assert plain[0] == 58 and grouped[0] == 58 and grouped[1] == 123.0 and np.all(grouped[2] == 7.0)
    finally:
        f.close()
    f, X, th0, z = _failing_fit(False)
    try:
        slope = np.array([0.0, 0.3, -0.2])
        up = float((X[57] - X[40]) @ slope) > 0
        good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
        before = _bits(f, good, 65, cols=(4,))
        plain, grouped = _raw_value(f, bad, False), _raw_value(f, bad, True)
        assert plain[0] == 58 and grouped[0] == 58 and grouped[1] == 123.0 and np.all(grouped[2] == 7.0)
        for g in (False, True):
            with pytest.raises(_lib.CholeskyError) as e:
                (f.whiten_grouped_core if g else f.whiten_core)(bad, z)
            assert e.value.minor == 58
        after = _bits(f, good, 65, cols=(4,))                # the next calls on the handle are clean
        assert all(_same(a, b) for a, b in zip(before, after))
    finally:
        f.close()
    _report("failing block: code and failure word of the ungrouped entry", "n65 row 58", 0.0)


def _dirs(p):
    return np.eye(6 * p)[:4].reshape(4, 6, p)


def test_repeats_and_any_order_of_calls():
    """a grouped call repeated; a grouped call after the gradient, the information, a simulation, a cross-validation and a
    second set_groups; and those entries after a grouped call: always the bits of a fresh handle"""
    n, m, cap = 300, 10, 64
    th, Rz = problem(n)[2], problem(n)[7]
    group = tables(n, m, cap)[1]
    E = columns(n, 4)
    others = OrderedDict((("gradient", lambda f: f.neg2loglik_grad_core(th)), ("information", lambda f: f.fisher_core(th, _dirs(f.p))),
                          ("simulation", lambda f: (f.sim_core(th, E),)), ("cross-validation", lambda f: f.cv_core(th)),
                          ("set_groups", lambda f: ([v for _, v in sorted(f.set_groups(group).items())],))))

    def grouped(f):
        v, p = f.neg2loglik_core(th, grouped=True)
        Y, l = f.whiten_grouped_core(th, Rz)
        return v, p, Y, l

    def flat(out):
        return [np.asarray(o, dtype=float) for o in out if o is not None]

    fresh = _grouped_fit(n, m, cap)
    try:
        want = flat(grouped(fresh))
        assert all(_same(a, b) for a, b in zip(want, flat(grouped(fresh))))            # repeated
    finally:
        fresh.close()
    want_other = {}
    for name, call in others.items():
        f = _grouped_fit(n, m, cap)
        try:
            want_other[name] = flat(call(f))                                            # on a fresh handle
            got = flat(grouped(f))                                                      # the grouped calls after it
            assert all(_same(a, b) for a, b in zip(want, got)), name
        finally:
            f.close()
    f = _grouped_fit(n, m, cap)
    try:
        for name, call in others.items():
            grouped(f)
            got = flat(call(f))                                                         # after grouped calls
            assert len(got) == len(want_other[name]) and all(_same(a, b) for a, b in zip(want_other[name], got)), name
    finally:
        f.close()
    _report("bits: repeats, grouped calls between the other Vecchia entries", "n%d m%d cap%d" % (n, m, cap), 0.0)


def test_a_second_plan_replaces_the_first():
    n, m = 300, 10
    th = problem(n)[2]
    nn, group, wide = tables(n, m, 64)
    f = _grouped_fit(n, m, 64)
    try:
        first = f.groups_info()
        base = f.info()["bytes"]
        own = np.arange(n, dtype=np.int32)                   # every row a block of its own: closed for any table
        second = f.set_groups(own)
        assert second["blocks"] == n and second["pairs"] == GR.pairs_ungrouped(wide) and first["pairs"] < second["pairs"]
        assert f.info()["bytes"] - base == second["bytes"] - first["bytes"]
        _bits(f, th, n, cols=(5,))
        assert f.set_groups(group) == first
        _bits(f, th, n, cols=(5,))
    finally:
        f.close()


def test_refusals_carry_messages():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n, m = 65, 10
    locs, X, th, z = problem(n)[:4]
    nn, group, wide = tables(n, m, 64)
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    val, parts, out = ctypes.c_double(0.0), np.zeros(3), np.zeros((n, 2), order="F")
    zf = np.asfortranarray(z)
    g32 = np.ascontiguousarray(group, dtype=np.int32)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    taper = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, 0.2)
    plain = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    narrow = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        L = plain._L
        # a handle without a plan
        assert L.cocons_neg2loglik_vecchia_grouped(plain._h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts)) == -1
        assert _lib.last_error().startswith("cocons_neg2loglik_vecchia_grouped: the handle has no plan")
        assert L.cocons_vecchia_whiten_grouped(plain._h, host._p(T), 2, host._p(zf), host._p(out), None) == -1
        assert _lib.last_error().startswith("cocons_vecchia_whiten_grouped: the handle has no plan")
        with pytest.raises(_lib.CoconsHipError, match="no plan"):
            plain.groups_info()
        # the other kinds of handle
        for h in (dense, taper):
            assert L.cocons_neg2loglik_vecchia_grouped(h._h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts)) < 0
            assert _lib.last_error().startswith("cocons_neg2loglik_vecchia_grouped: not a Vecchia fit")
            assert L.cocons_vecchia_whiten_grouped(h._h, host._p(T), 2, host._p(zf), host._p(out), None) < 0
            assert _lib.last_error().startswith("cocons_vecchia_whiten_grouped: not a Vecchia fit")
            assert L.cocons_vecchia_set_groups(h._h, host._ip(g32)) < 0
            assert _lib.last_error().startswith("cocons_vecchia_set_groups: not a Vecchia fit")
        # null arguments
        assert L.cocons_vecchia_set_groups(plain._h, None) == -1 and "null argument" in _lib.last_error()
        assert L.cocons_vecchia_set_groups(None, host._ip(g32)) == -1 and "null fit handle" in _lib.last_error()
        plain.set_groups(group)
        assert L.cocons_neg2loglik_vecchia_grouped(plain._h, None, host._p(mean), ctypes.byref(val), host._p(parts)) == -1
        assert _lib.last_error() == "cocons_neg2loglik_vecchia_grouped: null argument"
        assert L.cocons_neg2loglik_vecchia_grouped(plain._h, host._p(T), host._p(mean), None, host._p(parts)) == -1
        assert L.cocons_vecchia_whiten_grouped(plain._h, host._p(T), 2, None, host._p(out), None) == -1
        assert _lib.last_error() == "cocons_vecchia_whiten_grouped: null argument"
        assert L.cocons_vecchia_whiten_grouped(plain._h, host._p(T), 0, host._p(zf), host._p(out), None) == -1
        assert "c = 0" in _lib.last_error()
        assert L.cocons_vecchia_whiten_grouped(None, host._p(T), 2, host._p(zf), host._p(out), None) == -1

        # the closure check: the first offending row is named, and the former plan stays
        def refused(f, g, *words):
            with pytest.raises(_lib.CoconsHipError) as e:
                f.set_groups(g)
            assert all(w in str(e.value) for w in ("cocons_vecchia_set_groups:",) + words), str(e.value)

        refused(narrow, group, "row %d " % GR.closed(nn, group), "not closed")          # a partition the table is not closed under
        refused(plain, np.zeros(n, dtype=np.int32), "block of row 1 ", "more than 64 rows")   # a block of 65 rows
        bad = group.copy()
        bad[3] = n
        refused(plain, bad, "group[3]")
        assert plain.groups_info()["blocks"] == GR.plan(wide, group)["blocks"]
    finally:
        for h in (dense, taper, plain, narrow):
            h.close()
    # a member row with one neighbour too few, and with one too many
    pl = GR.plan(wide, group)
    size = np.diff(pl["off"])
    big = max((b for b in range(pl["blocks"]) if bin(pl["mask"][b] >> 1).count("1") >= 2 and size[b] <= 60), key=lambda b: pl["off"][b + 1])
    last = int(pl["rows"][pl["off"][big + 1] - 1])
    few = wide.copy(order="F")
    few[last, 0] = 0
    inside = set(pl["rows"][pl["off"][big]:pl["off"][big + 1]].tolist())
    extra = next(v for v in range(last) if v not in inside)
    many = np.asfortranarray(np.hstack([wide, np.zeros((n, 1), dtype=np.int32)]))[:, :63]
    assert pl["pos"][last] < many.shape[1] and many[last, pl["pos"][last]] == 0
    many[last, pl["pos"][last]] = extra + 1
    for tab in (few, many):
        f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, tab)
        try:
            with pytest.raises(_lib.CoconsHipError) as e:
                f.set_groups(group)
            assert "cocons_vecchia_set_groups: row %d " % GR.closed(tab, group) in str(e.value)
        finally:
            f.close()
    _report("refusals", "n65", 0.0)


def test_a_searched_handle_takes_groups_and_the_host_forms_take_the_keyword():
    """cocons_fit_create_vecchia_knn keeps its table on the device alone: set_groups downloads it for the check.  A single row
    per block is closed for any table.  And the three host objectives with grouped=True give the bits of grouped=False on the
    same handle."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m = 300, 10
    locs, X, th, z = problem(n)[:4]
    f = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, m)
    try:
        assert f.set_groups(np.arange(n))["blocks"] == n
        _bits(f, th, n, cols=(5,))
    finally:
        f.close()
    pp = wl.par_pos_full()
    tv = wl.theta_vector_from_lists(th, pp)
    lam = (0.0, 0.0, 0.0)
    nn, group, wide = tables(n, m, 64)
    f = _grouped_fit(n, m, 64)
    try:
        for g in (False, True):
            got = (ca.GetNeg2loglikelihoodVecchia(tv, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f, grouped=g),
                   ca.GetNeg2loglikelihoodVecchiaProfile(tv, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=f, grouped=g),
                   ca.GetNeg2loglikelihoodVecchiaREML(tv, pp, nn, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f, grouped=g))
            if not g:
                want = got
        assert got == want
        own = ca.GetNeg2loglikelihoodVecchia(tv, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, grouped=True)   # its own handle
        assert own == want[0]
    finally:
        f.close()
    _report("bits: a searched handle, the host objectives", "n%d m%d" % (n, m), 0.0)
