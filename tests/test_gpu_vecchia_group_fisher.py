"""The grouped Vecchia information on the GPU (cocons_fisher_vecchia_grouped), on the problem of
test_gpu_dense_sizes.problem and the tables of tests/group_reference.py.

PARITY: info against cocons_fisher_vecchia on the same handle -- the same model, summed in another order -- within TOL = 1e-7
in fisher_reference.metric (4t's bound), info_mean within MEAN_TOL = 1e-10 of its largest entry; the same bounds against the
numpy statement of the block form where that stays within a second; one block of 64 members against cocons_fisher_dense within
DENSE_TOL = 1e-9.  BITS: every output against itself across calls, launch orders and sequences of other entries, and symmetry
-- no tolerance.  Every comparison prints its worst error on a line that starts with `vecchia-group-fisher-report`; the
measured figures stand in tests/golden/VECCHIA_GROUP_FISHER_REPORT.md."""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
import grad_reference as GRD  # noqa: E402
import group_reference as GR  # noqa: E402
import vecchia_group_fisher_reference as VGF  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402
from test_gpu_vecchia import _theta  # noqa: E402
from test_gpu_vecchia_fisher import DENSE_TOL, MEAN_TOL, TOL, _raw, dirs19, mixes  # noqa: E402
from test_gpu_vecchia_grad import _coincident  # noqa: E402
from test_gpu_vecchia_group import CAPS, MS, _failing_fit, _grouped_fit, _hand_fit, _same, columns, tables  # noqa: E402
from test_gpu_vecchia_group_grad import _pair_in_one_block, _with_order  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 65, 300)


def _report(what, case, err):
    print("vecchia-group-fisher-report gpu | %s | %s | %.2e" % (what, case, err))


def _errs(got, want):
    return FR.metric(got[0], want[0]), float(np.max(np.abs(got[1] - want[1])) / np.max(np.abs(want[1])))


def _check(f, th, D, case, statement=None, scaling=None):
    """PARITY with the ungrouped entry on the handle (and the statement when given), symmetry to the bit; returns the grouped
    result"""
    got = f.fisher_core(th, D, grouped=True)
    plain = f.fisher_core(th, D)
    assert _same(got[0], got[0].T) and _same(got[1], got[1].T), case
    errs = _errs(got, plain)
    _report("info (metric) against the ungrouped entry on the handle", case, errs[0])
    _report("info_mean (relative) against the ungrouped entry on the handle", case, errs[1])
    assert errs[0] <= TOL and errs[1] <= MEAN_TOL, (case, errs)
    if statement is not None:
        serrs = _errs(got, statement)
        _report("info (metric) against the statement of the block form", case, serrs[0])
        _report("info_mean (relative) against the statement of the block form", case, serrs[1])
        assert serrs[0] <= TOL and serrs[1] <= MEAN_TOL, (case, serrs)
    if scaling is not None:
        n, r = f.n, f.r
        gap = abs(got[0][scaling, scaling] - r * n / 2)
        _report("I(v_s, v_s) - r n / 2, over n", case, gap / n)
        assert gap <= 1e-9 * n, (case, gap)
    return got


def _statement(th, locs, X, r, wide, group, D, sl=None):
    from cocons_amd import host, workloads as wl
    return VGF.statement(host.theta_table(th), locs, X, tuple(sl or wl.SMOOTH_LIMITS), D, wide, group, r)


@functools.lru_cache(maxsize=None)
def reference(n, m, cap):
    locs, X, th, z = problem(n)[:4]
    nn, group, wide = tables(n, m, cap)
    out = _statement(th, locs, X, z.shape[1], wide, group, dirs19(X.shape[1]))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_greedy_groups(n, m, cap):
    """the Bessel branch at a free smoothness (theta_full), the 6 p unit tables and the scaling direction (19 at p = 3: two
    groups of directions): blocks of 1 .. cap rows, one member to many -- more than a chunk of members at cap 64 --, pair
    walks of one pass and of several"""
    th = problem(n)[2]
    p = problem(n)[1].shape[1]
    f = _grouped_fit(n, m, cap)
    try:
        _check(f, th, dirs19(p), "n%d m%d cap%d blocks%d ndir%d" % (n, m, cap, f.groups_info()["blocks"], 6 * p + 1),
               statement=reference(n, m, cap), scaling=6 * p)
    finally:
        f.close()


@pytest.mark.parametrize("ndir", (1, 7, 17, 19))
def test_numbers_of_directions(ndir):
    """one direction (a group of four with one slot used), a partly filled group of eight, one more than a group of sixteen,
    and the unit tables with the scaling direction; the largest block has more members than any chunk holds (mc <= 16), so
    the Gram is summed over member chunks"""
    n, m, cap = 300, 30, 64
    locs, X, th, z = problem(n)[:4]
    nn, group, wide = tables(n, m, cap)
    pl = GR.plan(wide, group)
    assert max(bin(k).count("1") for k in pl["mask"]) > 16
    D = dirs19(3) if ndir == 19 else mixes(ndir)
    f = _grouped_fit(n, m, cap)
    try:
        _check(f, th, D, "n%d m%d cap%d ndir%d" % (n, m, cap, ndir),
               statement=reference(n, m, cap) if ndir == 19 else _statement(th, locs, X, z.shape[1], wide, group, D),
               scaling=18 if ndir == 19 else 0)
    finally:
        f.close()


@pytest.mark.parametrize("nu,slopes", ((0.5, False), (1.5, False), (2.5, False), (1.0, True)))
def test_closed_forms_and_the_bessel_branch_at_a_fixed_smoothness(nu, slopes):
    """(the free smoothness is every other test here)"""
    from cocons_amd import host
    n, m, cap = 300, 30, 64
    locs, X, th0, z = problem(n)[:4]
    th = _theta(th0) if slopes else _theta(th0, smooth=np.zeros(3))
    want = "geom" if slopes else {0.5: "half", 1.5: "threehalf", 2.5: "fivehalf"}[nu]
    assert GRD.select_mode(host.theta_table(th), (nu, nu))[0] == want
    nn, group, wide = tables(n, m, cap)
    D = mixes(7)
    f = _grouped_fit(n, m, cap, smooth_limits=(nu, nu))
    try:
        case = "nu%.1f%s n%d m%d cap%d" % (nu, " bessel" if slopes else "", n, m, cap)
        _check(f, th, D, case, statement=_statement(th, locs, X, z.shape[1], wide, group, D, (nu, nu)), scaling=0)
        got = f.fisher_core(th, dirs19(3), grouped=True)
        assert np.all(got[0][12:15] == 0.0) and np.all(got[0][:, 12:15] == 0.0)      # no smooth row at a fixed smoothness
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
        _check(f, th, dirs19(p), "n%d m%d cap%d r%d p%d" % (n, m, cap, r, p),
               statement=_statement(th, locs, X, r, wide, group, dirs19(p)), scaling=6 * p)
    finally:
        f.close()


def test_one_block_of_64_members_is_the_dense_information():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 64
    locs, X, th, z = (a[:n] if i != 2 else a for i, a in enumerate(problem(65)[:4]))
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    try:
        info = f.set_groups(np.zeros(n, dtype=np.int32))
        assert (info["blocks"], info["maxrows"], info["pairs"]) == (1, 64, 2016)
        want = dense.fisher_core(th, dirs19(3))
        got = _check(f, th, dirs19(3), "one block of 64 members n64", scaling=18)
    finally:
        dense.close()
        f.close()
    errs = _errs(got, want)
    _report("one block of 64 members against cocons_fisher_dense, info (metric)", "n64", errs[0])
    _report("one block of 64 members against cocons_fisher_dense, info_mean (relative)", "n64", errs[1])
    assert errs[0] <= DENSE_TOL and errs[1] <= DENSE_TOL, errs


def test_hand_made_partitions():
    """a block of 64 rows with a single member and blocks of one row; members interleaved with rows that are not, and a
    member at position 0 inside a larger block"""
    from cocons_amd import host
    n = 300
    locs, X, th, z = problem(n)[:4]
    r = z.shape[1]
    nn = np.zeros((n, 63), dtype=np.int32, order="F")
    nn[:, :3] = host.vecchia_neighbours(locs, 3)
    nn[199] = host.vecchia_neighbours(locs[:200], 63)[199]
    group = np.arange(n, dtype=np.int32)
    f, wide, pl = _hand_fit(n, nn, group)
    try:
        assert pl["maxrows"] == 64 and pl["mask"][199] == 1 << 63 and pl["blocks"] == n
        _check(f, th, dirs19(3), "64 rows with one member, blocks of one row n%d" % n,
               statement=_statement(th, locs, X, r, wide, group, dirs19(3)), scaling=18)
    finally:
        f.close()
    nn = host.vecchia_neighbours(locs, 4)
    stride = (np.arange(n) % 7 + 7 * (np.arange(n) // 49)).astype(np.int32)
    f, wide, pl = _hand_fit(n, nn, stride)
    try:
        first = pl["block"][0]
        assert pl["pos"][0] == 0 and pl["off"][first + 1] - pl["off"][first] > 1 and pl["mask"][first] & 1
        assert any((m >> q) & 7 == 5 for m in pl["mask"] for q in range(62))
        _check(f, th, dirs19(3), "interleaved members, a member at position 0 n%d blocks%d" % (n, pl["blocks"]),
               statement=_statement(th, locs, X, r, wide, stride, dirs19(3)), scaling=18)
    finally:
        f.close()


def test_a_coincident_pair_of_sites_inside_a_block():
    """observation 58 on the coordinates of observation 41 (u <= eps), in one block with the rows 61 and 65"""
    locs, X, th, z, nn = _coincident()
    f, wide, pl = _pair_in_one_block(locs, X, z, nn, (57, 60, 64))
    try:
        b = pl["block"][57]
        assert 40 in pl["rows"][pl["off"][b]:pl["off"][b + 1]] and bin(pl["mask"][b]).count("1") == 3
        group = np.arange(65, dtype=np.int32)
        group[[60, 64]] = 57
        _check(f, th, dirs19(3), "coincident pair inside a block n65 m10",
               statement=_statement(th, locs, X, z.shape[1], wide, group, dirs19(3)), scaling=18)
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
        group = np.arange(n, dtype=np.int32)
        group[[55, 60]] = 50
        _check(f, th, dirs19(3), "far pair inside a block n65 m10",
               statement=_statement(th, locs, X, z.shape[1], wide, group, dirs19(3)), scaling=18)
    finally:
        f.close()


def test_more_blocks_than_one_chunk():
    """12 289 blocks of one member each at m = 1, 16 directions and p = 3 -- one more than the 12 288 records of a launch --,
    a closed form: against the ungrouped entry on the handle, and the bits repeat"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m = 12289, 1
    rng = np.random.default_rng(33)
    locs = np.column_stack([np.sort(rng.uniform(0, 40, size=n)), rng.uniform(0, 0.2, size=n)])
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    z = rng.standard_normal((n, 1))
    nn = np.zeros((n, m), dtype=np.int32, order="F")
    nn[1:, 0] = np.arange(1, n)
    th = _theta(wl.theta_full(scale0=np.log(0.2)), smooth=np.zeros(3), mean=[0.3, -0.15, 0.2])
    D = mixes(16)
    f = ca.CoconsVecchiaFit(locs, X, z, (1.5, 1.5), nn)
    try:
        assert f.set_groups(np.arange(n, dtype=np.int32))["blocks"] == n
        got = _check(f, th, D, "n%d m%d blocks%d nu1.5 ndir16 (two chunks)" % (n, m, n), scaling=0)
        again = f.fisher_core(th, D, grouped=True)
        assert _same(got[0], again[0]) and _same(got[1], again[1])
    finally:
        f.close()


def _flat(out):
    return [np.asarray(o, dtype=float) for o in out if o is not None]


def test_bits_repeat_whatever_the_launch_order_and_the_calls_before():
    """the outputs repeat across calls, with COCONS_VECCHIA_GROUP_ORDER=0 and 1, and after value, whitening, both gradients,
    the ungrouped information, simulation, cross-validation and a second set_groups on the handle; those entries -- the
    ungrouped information, the grouped value and the grouped gradient among them -- keep their fresh-handle bits with the
    grouped information called between them"""
    n, m, cap = 300, 10, 64
    locs, X, th, z = problem(n)[:4]
    Rz = problem(n)[7]
    group = tables(n, m, cap)[1]
    E = columns(n, 4)

    def grouped(f):
        return _flat(f.fisher_core(th, dirs19(3), grouped=True)) + _flat(f.fisher_core(th, mixes(7), grouped=True))

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
                          ("gradient", lambda f: f.neg2loglik_grad_core(th)),
                          ("grouped gradient", lambda f: f.neg2loglik_grad_core(th, grouped=True)),
                          ("information", lambda f: f.fisher_core(th, dirs19(3))),
                          ("simulation", lambda f: (f.sim_core(th, E),)), ("cross-validation", lambda f: f.cv_core(th)),
                          ("set_groups", lambda f: ([v for _, v in sorted(f.set_groups(group).items())],))))
    want_other = {}
    for name, call in others.items():
        f = _grouped_fit(n, m, cap)
        try:
            want_other[name] = _flat(call(f))                                               # on a fresh handle
            assert all(_same(a, b) for a, b in zip(want, grouped(f))), name                 # the grouped information after it
        finally:
            f.close()
    f = _grouped_fit(n, m, cap)
    try:
        for name, call in others.items():
            grouped(f)
            got = _flat(call(f))                                                            # after grouped informations
            assert len(got) == len(want_other[name]) and all(_same(a, b) for a, b in zip(want_other[name], got)), name
        assert all(_same(a, b) for a, b in zip(want, grouped(f)))                           # after the whole sequence
    finally:
        f.close()
    _report("bits: repeats, both launch orders, between the other entries", "n%d m%d cap%d" % (n, m, cap), 0.0)


def test_failing_block_in_the_middle_of_a_group():
    """the failing case of test_gpu_vecchia_group: the pivot of row 58 fails with rows behind it in the block.  The
    ungrouped entry's code, the outputs left alone, and the next call clean"""
    f, X, th0, z = _failing_fit(False)
    try:
        slope = np.array([0.0, 0.3, -0.2])
        up = float((X[57] - X[40]) @ slope) > 0
        good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
        before = _flat(f.fisher_core(good, dirs19(3), grouped=True))
        plain, grouped = _raw(f, bad, dirs19(3)), _raw(f, bad, dirs19(3), "cocons_fisher_vecchia_grouped")
        assert plain[0] == 58 and grouped[0] == 58
        assert np.all(grouped[1] == 7.0) and np.all(grouped[2] == 7.0)
        after = _flat(f.fisher_core(good, dirs19(3), grouped=True))
        assert all(_same(a, b) for a, b in zip(before, after))
    finally:
        f.close()
    _report("failing block: code of the ungrouped entry", "n65 row 58", 0.0)


def test_refusals_carry_messages():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    entry = "cocons_fisher_vecchia_grouped"
    n, m = 65, 10
    locs, X, th, z = problem(n)[:4]
    wide = tables(n, m, 64)[2]
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    taper = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, 0.2)
    plain = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    try:
        rc, info, im = _raw(plain, th, dirs19(3), entry)
        assert rc == -1 and np.all(info == 7.0) and np.all(im == 7.0)
        assert _lib.last_error().startswith(entry + ": the handle has no plan")
        with pytest.raises(_lib.CoconsHipError, match="no plan"):
            plain.fisher_core(th, dirs19(3), grouped=True)
        for h in (dense, taper):
            rc, info, im = _raw(h, th, dirs19(3), entry)
            assert rc < 0 and np.all(info == 7.0) and np.all(im == 7.0)
            assert _lib.last_error().startswith(entry + ": not a Vecchia fit")
        plain.set_groups(tables(n, m, 64)[1])
        D = dirs19(3).copy()
        D[4, 2, 1] = np.inf
        rc, info, im = _raw(plain, th, D, entry)
        assert rc == -1 and np.all(info == 7.0) and np.all(im == 7.0)
        assert _lib.last_error().startswith(entry + ": direction 4 has a non-finite entry")
        rc, info, im = _raw(plain, th, dirs19(3), "cocons_fisher_dense")           # still refused on a Vecchia handle
        assert rc == -1 and np.all(info == 7.0)
        assert _lib.last_error().startswith("cocons_fisher_dense: not available on a Vecchia fit")
        info_only = np.full(19 * 19, 7.0)                # info_mean may be NULL
        T, D = host.theta_table(th), np.ascontiguousarray(dirs19(3).reshape(19, 18))
        assert getattr(plain._L, entry)(plain._h, host._p(T), 19, host._p(D), host._p(info_only), None) == 0
        assert _same(info_only.reshape(19, 19), plain.fisher_core(th, dirs19(3), grouped=True)[0])
    finally:
        for h in (dense, taper, plain):
            h.close()


def test_the_handle_holds_the_bytes_of_the_ungrouped_call():
    n, m, cap = 300, 30, 64
    th = problem(n)[2]
    f, g = _grouped_fit(n, m, cap), _grouped_fit(n, m, cap)
    try:
        assert f.info()["bytes"] == g.info()["bytes"]
        f.fisher_core(th, dirs19(3), grouped=True)
        g.fisher_core(th, dirs19(3))
        first = f.info()["bytes"]
        assert first == g.info()["bytes"]
        f.fisher_core(th, dirs19(3))
        f.fisher_core(th, mixes(7), grouped=True)
        assert f.info()["bytes"] == first
    finally:
        f.close()
        g.close()


def test_host_entry():
    """getFisher_vecchia(..., grouped=True) against grouped=False on the same handle -- the expanded table, the same model --
    and on a handle of its own"""
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    n, m, cap = 300, 10, 64
    locs, X, th, z = problem(n)[:4]
    nn = tables(n, m, cap)[0]
    pp = OrderedDict((k, [True] * 3) for k in host.ASPECTS)
    par = wl.theta_vector_from_lists(th, pp)
    f = _grouped_fit(n, m, cap)
    try:
        out = {g: ca.getFisher_vecchia(par, pp, locs, X, wl.SMOOTH_LIMITS, z, n, nn, fit=f, grouped=g) for g in (False, True)}
    finally:
        f.close()
    own = ca.getFisher_vecchia(par, pp, locs, X, wl.SMOOTH_LIMITS, z, n, nn, grouped=True)
    gap = FR.metric(out[True], out[False])
    _report("getFisher_vecchia grouped against ungrouped on the expanded table (metric)", "n%d m%d cap%d P%d" % (n, m, cap, par.size), gap)
    assert _same(own, out[True]) and _same(own, own.T) and own.shape == (par.size, par.size) and gap <= TOL
    ev = np.linalg.eigvalsh(own)
    assert ev[0] >= -1e-12 * ev[-1]
