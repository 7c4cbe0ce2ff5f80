"""The grouped Vecchia gradient on the GPU (cocons_neg2loglik_grad_vecchia_grouped), on the problem of
test_gpu_dense_sizes.problem and the tables of tests/group_reference.py.

Three kinds of comparison.  BITS: sum_logliks and parts against the grouped value entry (and so the ungrouped one), and every
output against itself across calls, launch orders and sequences of other entries -- no tolerance.  GRADIENT: grad_theta,
grad_quad and grad_mean against the ungrouped gradient entry on the same handle -- the same model, summed in another order --
and against the numpy statement on the expanded table, both within GRAD_TOL = 1e-7 of tests/test_gpu_vecchia_grad.py, relative
to the largest magnitude.  DIFFERENCES: against Richardson differences of the grouped value entry within FD_TOL = 1e-6.  Every
test prints its worst deviation on a line that starts with `vecchia-group-grad-report`; the measured figures stand in
tests/golden/VECCHIA_GROUP_GRAD_REPORT.md."""
import ctypes
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference as GRD  # noqa: E402
import group_reference as GR  # noqa: E402
import vecchia_grad_reference as VG  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402
from test_gpu_vecchia import _theta  # noqa: E402
from test_gpu_vecchia_grad import FD_TOL, GRAD_TOL, _coincident, _differences  # noqa: E402
from test_gpu_vecchia_group import CAPS, COLS, MS, _dirs, _failing_fit, _grouped_fit, _hand_fit, _same, columns, tables  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 65, 300)


def _report(what, case, err):
    print("vecchia-group-grad-report gpu | %s | %s | %.2e" % (what, case, err))


def _rel(got, want, scale=None):
    want = np.asarray(want, dtype=float)
    scale = want if scale is None else np.asarray(scale, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(scale))), 1e-300))


def _grad_errs(got, want):
    """table, quad (relative to the table) and mean of two (value, parts, table, quad, mean) results"""
    errs = [_rel(got[2], want[2]), _rel(got[3], want[3], want[2])]
    if want[4] is not None:
        errs.append(_rel(got[4], want[4]))
    return errs


def _check(f, th, case, B=None, statement=None):
    """BITS of value and parts, GRADIENT against the ungrouped entry on the handle (and the statement when given); returns the
    grouped result"""
    got = f.neg2loglik_grad_core(th, B=B, grouped=True)
    plain = f.neg2loglik_grad_core(th, B=B)
    assert got[0] == plain[0] and _same(got[1], plain[1]), (case, got[0] - plain[0])
    if B is None:
        v, parts = f.neg2loglik_core(th, grouped=True)
        assert got[0] == v and _same(got[1], parts), (case, got[0] - v)
    else:
        assert got[4] is None and got[1].size == 1 + B.shape[1]
    errs = _grad_errs(got, plain)
    _report("table quad mean against the ungrouped entry on the handle", case, max(errs))
    assert max(errs) < GRAD_TOL, (case, errs)
    if statement is not None:
        serrs = [abs(got[0] - statement[0]) / abs(statement[0])] + _grad_errs(got, statement)
        _report("value table quad mean against the statement on the expanded table", case, max(serrs))
        assert serrs[0] < 1e-8 and max(serrs[1:]) < GRAD_TOL, (case, serrs)
    return got


def _statement(th, locs, X, z, wide, sl=None, B=None):
    from cocons_amd import host, workloads as wl
    return VG.neg2loglik_grad(host.theta_table(th), th["mean"], locs, X, z, tuple(sl or wl.SMOOTH_LIMITS), wide, B=B)


@functools.lru_cache(maxsize=None)
def reference(n, m, cap):
    locs, X, th, z = problem(n)[:4]
    out = _statement(th, locs, X, z, tables(n, m, cap)[2])
    for a in out[1:]:
        a.setflags(write=False)
    return out


class _GroupedValue:
    """the handle as `_differences` sees it: its value entry is the grouped one"""

    def __init__(self, f):
        self.f = f

    def neg2loglik_core(self, th):
        return self.f.neg2loglik_core(th, grouped=True)


def _check_differences(f, th, got, case, skip_smooth=False):
    tab, gm = _differences(_GroupedValue(f), th, skip_smooth)
    scale = max(np.max(np.abs(tab)), np.max(np.abs(gm)))
    err = max(np.max(np.abs(got[2] - tab)), np.max(np.abs(got[4] - gm))) / scale
    _report("against differences of the grouped value entry", case, err)
    assert err < FD_TOL, (case, err)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_greedy_groups(n, m, cap):
    """the Bessel branch at a free smoothness (theta_full): blocks of 1 .. cap rows, one member to many, pair walks of one
    pass and of several; the statement on the expanded table where it stays within a second (n <= 65, and n = 300 at m = 10)"""
    th = problem(n)[2]
    f = _grouped_fit(n, m, cap)
    try:
        ref = reference(n, m, cap) if (n <= 65 or m == 10) else None
        _check(f, th, "n%d m%d cap%d blocks%d" % (n, m, cap, f.groups_info()["blocks"]), statement=ref)
    finally:
        f.close()


@pytest.mark.parametrize("nu,slopes", ((0.5, False), (1.5, False), (2.5, False), (1.0, True)))
def test_closed_forms_and_the_bessel_branch_at_a_fixed_smoothness(nu, slopes):
    from cocons_amd import host
    n, m, cap = 300, 30, 64
    locs, X, th0, z = problem(n)[:4]
    th = _theta(th0) if slopes else _theta(th0, smooth=np.zeros(3))
    want = "geom" if slopes else {0.5: "half", 1.5: "threehalf", 2.5: "fivehalf"}[nu]
    assert GRD.select_mode(host.theta_table(th), (nu, nu))[0] == want
    f = _grouped_fit(n, m, cap, smooth_limits=(nu, nu))
    try:
        case = "nu%.1f%s n%d m%d cap%d" % (nu, " bessel" if slopes else "", n, m, cap)
        got = _check(f, th, case)
        assert np.all(got[2][4] == 0.0) and np.all(got[3][4] == 0.0)
        _check_differences(f, th, got, case, skip_smooth=True)
    finally:
        f.close()


def test_free_smoothness_against_differences():
    n, m, cap = 300, 30, 64
    th = problem(n)[2]
    f = _grouped_fit(n, m, cap)
    try:
        got = _check(f, th, "free smoothness n%d m%d cap%d" % (n, m, cap))
        assert np.any(got[2][4] != 0.0)
        _check_differences(f, th, got, "free smoothness n%d m%d cap%d" % (n, m, cap))
    finally:
        f.close()


@pytest.mark.parametrize("c", COLS)
def test_callers_columns(c):
    """B given: c = 1, 4, 5 and 9 -- the last group of four of the substitution full, partial and single"""
    n, m, cap = 300, 10, 64
    locs, X, th, z = problem(n)[:4]
    B = columns(n, c)
    f = _grouped_fit(n, m, cap)
    try:
        got = _check(f, th, "B c%d n%d m%d cap%d" % (c, n, m, cap), B=B,
                     statement=_statement(th, locs, X, z, tables(n, m, cap)[2], B=B) if c in (1, 5) else None)
        Y, logd = f.whiten_grouped_core(th, B)
        assert abs(got[1][0] - np.sum(logd)) <= 1e-12 * max(abs(np.sum(logd)), 1.0) and _rel(got[1][1:], np.sum(Y * Y, axis=0)) <= 1e-12
    finally:
        f.close()


@pytest.mark.parametrize("r,p", ((1, 3), (3, 3), (1, 1), (3, 1)))
def test_realisations_and_design_widths(r, p):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m, cap = 65, 10, 17
    locs, X, th0, z = problem(n)[:4]
    z = np.asfortranarray(np.column_stack([z, np.random.default_rng(3).standard_normal(n)])[:, :r])
    X = np.asfortranarray(X[:, :p])
    th = OrderedDict((k, np.array(v[:p], copy=True)) for k, v in th0.items())
    nn, group, wide = tables(n, m, cap)
    f = ca.CoconsVecchiaFit.from_groups(locs, X, z, wl.SMOOTH_LIMITS, nn, cap)
    try:
        case = "n%d m%d cap%d r%d p%d" % (n, m, cap, r, p)
        got = _check(f, th, case, statement=_statement(th, locs, X, z, wide))
        _check_differences(f, th, got, case)
    finally:
        f.close()


def test_one_block_of_64_member_rows_is_the_dense_gradient():
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    n = 64
    locs, X, th, z = (a[:n] if i != 2 else a for i, a in enumerate(problem(65)[:4]))
    fv, gt, gm = GRD.neg2loglik_grad(host.theta_table(th), th["mean"], locs, X, z, wl.SMOOTH_LIMITS)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    try:
        info = f.set_groups(np.zeros(n, dtype=np.int32))
        assert (info["blocks"], info["maxrows"], info["pairs"]) == (1, 64, 2016)
        got = _check(f, th, "one block of 64 members n64")
    finally:
        f.close()
    errs = (abs(got[0] - fv) / abs(fv), _rel(got[2], gt), _rel(got[4], gm))
    _report("one block of 64 members against the dense gradient", "n64", max(errs))
    assert errs[0] < 1e-8 and max(errs[1:]) < GRAD_TOL, errs


def test_hand_made_partitions():
    """a block of 64 rows with a single member and blocks of one row; members interleaved with rows that are not, and a
    member at position 0 inside a larger block"""
    from cocons_amd import host
    n = 300
    locs, X, th, z = problem(n)[:4]
    nn = np.zeros((n, 63), dtype=np.int32, order="F")
    nn[:, :3] = host.vecchia_neighbours(locs, 3)
    nn[199] = host.vecchia_neighbours(locs[:200], 63)[199]
    f, wide, pl = _hand_fit(n, nn, np.arange(n, dtype=np.int32))
    try:
        assert pl["maxrows"] == 64 and pl["mask"][199] == 1 << 63 and pl["blocks"] == n
        _check(f, th, "64 rows with one member, blocks of one row n%d" % n, statement=_statement(th, locs, X, z, wide))
    finally:
        f.close()
    nn = host.vecchia_neighbours(locs, 4)
    stride = (np.arange(n) % 7 + 7 * (np.arange(n) // 49)).astype(np.int32)
    f, wide, pl = _hand_fit(n, nn, stride)
    try:
        first = pl["block"][0]
        assert pl["pos"][0] == 0 and pl["off"][first + 1] - pl["off"][first] > 1 and pl["mask"][first] & 1
        assert any((m >> q) & 7 == 5 for m in pl["mask"] for q in range(62))
        _check(f, th, "interleaved members, a member at position 0 n%d blocks%d" % (n, pl["blocks"]),
               statement=_statement(th, locs, X, z, wide))
    finally:
        f.close()


def _pair_in_one_block(locs, X, z, nn, rows):
    """the grouped handle of the table nn with the 0-based `rows` in one block and every other row on its own"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = z.shape[0]
    group = np.arange(n, dtype=np.int32)
    group[list(rows)] = group[rows[0]]
    wide = ca.vecchia_group_table(nn, group)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    f.set_groups(group)
    return f, wide, GR.plan(wide, group)


def test_a_coincident_pair_of_sites_inside_a_block():
    """observation 58 on the coordinates of observation 41 (u <= eps), in one block with the rows 61 and 65"""
    locs, X, th, z, nn = _coincident()
    f, wide, pl = _pair_in_one_block(locs, X, z, nn, (57, 60, 64))
    try:
        b = pl["block"][57]
        assert 40 in pl["rows"][pl["off"][b]:pl["off"][b + 1]] and bin(pl["mask"][b]).count("1") == 3
        got = _check(f, th, "coincident pair inside a block n65 m10", statement=_statement(th, locs, X, z, wide))
        _check_differences(f, th, got, "coincident pair inside a block n65 m10")
    finally:
        f.close()


def test_a_far_pair_inside_a_block():
    """one site 70 units away from the others at a range of 0.2: u >= 706, the entry and its partials are zero"""
    from cocons_amd import host
    n, m = 65, 10
    locs, X, th, z = problem(n)[:4]
    locs = np.array(locs)
    locs[50] = (50.0, 50.0)
    nn = host.vecchia_neighbours(locs, m)
    f, wide, pl = _pair_in_one_block(locs, X, z, nn, (50, 55, 60))
    try:
        b = pl["block"][50]
        assert bin(pl["mask"][b]).count("1") == 3 and pl["off"][b + 1] - pl["off"][b] > 11
        _check(f, th, "far pair inside a block n65 m10", statement=_statement(th, locs, X, z, wide))
    finally:
        f.close()


def test_more_blocks_than_one_chunk():
    """33 000 blocks of one row each -- more than the 32 768 records of one launch --, a closed form and ten predecessors in
    a chain: against the ungrouped entry on the handle, and the bits repeat"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m = 33000, 10
    rng = np.random.default_rng(33)
    locs = np.column_stack([np.sort(rng.uniform(0, 40, size=n)), rng.uniform(0, 0.2, size=n)])
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    z = rng.standard_normal((n, 1))
    nn = np.zeros((n, m), dtype=np.int32, order="F")
    for j in range(m):
        nn[j + 1:, j] = np.arange(1, n - j)
    th = _theta(wl.theta_full(scale0=np.log(0.2)), smooth=np.zeros(3), mean=[0.3, -0.15, 0.2])
    f = ca.CoconsVecchiaFit(locs, X, z, (1.5, 1.5), nn)
    try:
        assert f.set_groups(np.arange(n, dtype=np.int32))["blocks"] == n
        got = _check(f, th, "n%d m%d blocks%d nu1.5 (two chunks)" % (n, m, n))
        again = f.neg2loglik_grad_core(th, grouped=True)
        assert got[0] == again[0] and all(_same(a, b) for a, b in zip(got[1:], again[1:]))
    finally:
        f.close()


def _flat(out):
    return [np.asarray(o, dtype=float) for o in out if o is not None]


def _with_order(value, make):
    old = os.environ.get("COCONS_VECCHIA_GROUP_ORDER")
    os.environ["COCONS_VECCHIA_GROUP_ORDER"] = value
    try:
        return make()
    finally:
        if old is None:
            del os.environ["COCONS_VECCHIA_GROUP_ORDER"]
        else:
            os.environ["COCONS_VECCHIA_GROUP_ORDER"] = old


def test_bits_repeat_whatever_the_launch_order_and_the_calls_before():
    """all outputs repeat across calls, with COCONS_VECCHIA_GROUP_ORDER=0 and 1, and after value, whitening, ungrouped
    gradient, information, simulation, cross-validation and a second set_groups on the handle; the ungrouped gradient and
    the dense gradient keep their bits beside it"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m, cap = 300, 10, 64
    locs, X, th, z = problem(n)[:4]
    Rz = problem(n)[7]
    group = tables(n, m, cap)[1]
    E = columns(n, 4)

    def grouped(f):
        return _flat(f.neg2loglik_grad_core(th, grouped=True)) + _flat(f.neg2loglik_grad_core(th, B=E, grouped=True))

    want = None
    for order in ("1", "0"):
        f = _with_order(order, lambda: _grouped_fit(n, m, cap))
        try:
            got = grouped(f)
            want = got if want is None else want
            assert all(_same(a, b) for a, b in zip(want, got)), order
            assert all(_same(a, b) for a, b in zip(want, grouped(f))), order                # repeated
        finally:
            f.close()
    others = OrderedDict((("value", lambda f: f.neg2loglik_core(th, grouped=True)), ("whiten", lambda f: f.whiten_grouped_core(th, Rz)),
                          ("gradient", lambda f: f.neg2loglik_grad_core(th)), ("information", lambda f: f.fisher_core(th, _dirs(f.p))),
                          ("simulation", lambda f: (f.sim_core(th, E),)), ("cross-validation", lambda f: f.cv_core(th)),
                          ("set_groups", lambda f: ([v for _, v in sorted(f.set_groups(group).items())],))))
    want_other = {}
    for name, call in others.items():
        f = _grouped_fit(n, m, cap)
        try:
            want_other[name] = _flat(call(f))                                               # on a fresh handle
            assert all(_same(a, b) for a, b in zip(want, grouped(f))), name                 # the grouped gradient after it
        finally:
            f.close()
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    f = _grouped_fit(n, m, cap)
    try:
        before = _flat(dense.neg2loglik_grad_core(th))
        for name, call in others.items():
            grouped(f)
            got = _flat(call(f))                                                            # after grouped gradients
            assert len(got) == len(want_other[name]) and all(_same(a, b) for a, b in zip(want_other[name], got)), name
        assert all(_same(a, b) for a, b in zip(before, _flat(dense.neg2loglik_grad_core(th))))
    finally:
        f.close()
        dense.close()
    _report("bits: repeats, both launch orders, between the other entries", "n%d m%d cap%d" % (n, m, cap), 0.0)


def _raw(f, th, grouped, B=None):
    from cocons_amd import host
    p = f.p
    val, parts = ctypes.c_double(123.0), np.full(8, 7.0)
    gt, gq, gm = np.full(6 * p, 7.0), np.full(6 * p, 7.0), np.full(p, 7.0)
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    entry = f._L.cocons_neg2loglik_grad_vecchia_grouped if grouped else f._L.cocons_neg2loglik_grad_vecchia
    if B is None:
        rc = entry(f._h, host._p(T), host._p(mean), 0, None, ctypes.byref(val), host._p(parts), host._p(gt), host._p(gq), host._p(gm))
    else:
        rc = entry(f._h, host._p(T), None, B.shape[1], host._p(B), ctypes.byref(val), host._p(parts), host._p(gt), host._p(gq), None)
    return rc, val.value, parts, gt, gq, gm


def test_failing_block_in_the_middle_of_a_group():
    """the failing case of test_gpu_vecchia_group: the pivot of row 58 fails with rows behind it in the block.  The
    ungrouped entry's code and failure word, the outputs left alone, and the next call clean"""
    f, X, th0, z = _failing_fit(False)
    try:
        slope = np.array([0.0, 0.3, -0.2])
        up = float((X[57] - X[40]) @ slope) > 0
        good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
        before = _flat(f.neg2loglik_grad_core(good, grouped=True))
        for B in (None, np.asfortranarray(z)):
            plain, grouped = _raw(f, bad, False, B), _raw(f, bad, True, B)
            assert plain[0] == 58 and grouped[0] == 58 and grouped[1] == 123.0
            assert all(np.all(a == 7.0) for a in grouped[2:])
        after = _flat(f.neg2loglik_grad_core(good, grouped=True))
        assert all(_same(a, b) for a, b in zip(before, after))
    finally:
        f.close()
    _report("failing block: code and failure word of the ungrouped entry", "n65 row 58", 0.0)


def test_refusals_carry_messages():
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    n, m = 65, 10
    locs, X, th, z = problem(n)[:4]
    wide = tables(n, m, 64)[2]
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    taper = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, 0.2)
    plain = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    try:
        rc, val, parts, gt, gq, gm = _raw(plain, th, True)
        assert rc == -1 and val == 123.0 and all(np.all(a == 7.0) for a in (parts, gt, gq, gm))
        assert _lib.last_error().startswith("cocons_neg2loglik_grad_vecchia_grouped: the handle has no plan")
        with pytest.raises(_lib.CoconsHipError, match="no plan"):
            plain.neg2loglik_grad_core(th, grouped=True)
        for h in (dense, taper):
            rc, val, parts, gt, gq, gm = _raw(h, th, True)
            assert rc < 0 and val == 123.0 and np.all(gt == 7.0)
            assert _lib.last_error().startswith("cocons_neg2loglik_grad_vecchia_grouped: not a Vecchia fit")
        plain.neg2loglik_grad_core(th)                  # (the handle stays usable)
    finally:
        for h in (dense, taper, plain):
            h.close()


def test_profile_and_reml_host_forms():
    """grouped=True against grouped=False on the same handle -- the expanded table, the same model"""
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    n, m, cap = 300, 10, 64
    locs, X, th, z = problem(n)[:4]
    nn = tables(n, m, cap)[0]
    pp = OrderedDict((k, [k != "mean"] * 3) for k in host.ASPECTS)
    tv = wl.theta_vector_from_lists(th, pp)
    pf = OrderedDict((k, [True] * 3) for k in host.ASPECTS)
    tvf = wl.theta_vector_from_lists(th, pf)
    lam = (0.0, 0.0, 0.0)
    f = _grouped_fit(n, m, cap)
    try:
        out = {}
        for g in (False, True):
            out[g] = (ca.GetNeg2loglikelihoodVecchiaProfile_grad(tv, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=f, grouped=g),
                      ca.GetNeg2loglikelihoodVecchiaREML_grad(tv, pp, nn, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f, grouped=g),
                      ca.GetNeg2loglikelihoodVecchia_grad(tvf, pf, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=f, grouped=g))
        own = ca.GetNeg2loglikelihoodVecchia_grad(tvf, pf, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, grouped=True)     # its own handle
    finally:
        f.close()
    assert all(a[0] == b[0] for a, b in zip(out[True], out[False]))            # the values to the bit
    assert own[0] == out[True][2][0] and _same(own[1], out[True][2][1])
    errs = [_rel(a[1], b[1]) for a, b in zip(out[True], out[False])]
    _report("profile reml plain (host forms) against the ungrouped forms on the expanded table", "n%d m%d cap%d" % (n, m, cap), max(errs))
    assert max(errs) < GRAD_TOL, errs
