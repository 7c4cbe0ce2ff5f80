"""The grouped U^-1, U' and cross-validation entries on the GPU (cocons_vecchia_unwhiten_grouped, cocons_sim_vecchia_grouped,
cocons_vecchia_whiten_t_grouped, cocons_cv_vecchia_grouped), on the problem of test_gpu_dense_sizes.problem and
the tables of tests/group_reference.py.

Every comparison is BITS (np.array_equal): a grouped entry against its twin on the same handle.  The coefficients are the only
thing the grouped entries compute differently -- one factorisation per block and a backward solve per member instead of one
factorisation per row -- and everything behind them reads the records alone, so equal outputs for the identity (every
coefficient of U), for 1, 4, 5 and 9 columns and for every fold class say that every record is equal.  Every test prints its
cases on lines that start with `vecchia-group-coef-report`; tests/golden/VECCHIA_GROUP_COEF_REPORT.md records what was run."""
import ctypes
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import vecchia_reference as VR  # noqa: E402
from test_gpu_dense_sizes import problem  # noqa: E402
from test_gpu_vecchia import _theta  # noqa: E402
from test_gpu_vecchia_fisher import dirs19  # noqa: E402
from test_gpu_vecchia_group import CAPS, COLS, MS, _failing_fit, _grouped_fit, _hand_fit, _same, columns, tables  # noqa: E402
from test_gpu_vecchia_group_grad import _with_order  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 65, 300)


def _report(what, case):
    print("vecchia-group-coef-report gpu | %s | %s | bits" % (what, case))


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _twins(f, th, n, cols=COLS, identity=False, folds=()):
    """every grouped entry against its twin on the handle f; returns the grouped outputs, flat"""
    out = []
    for c in cols:
        W = columns(n, c)
        x0, x1 = f.unwhiten_core(th, W), f.unwhiten_grouped_core(th, W)
        assert _same(x1, x0), ("unwhiten", c)
        t0, t1 = f.whiten_t_core(th, W), f.whiten_t_grouped_core(th, W)
        assert _all_same(t1, t0), ("whiten_t", c)
        out += [x1, *t1]
    if identity:
        t0, t1 = f.whiten_t_core(th, np.eye(n)), f.whiten_t_grouped_core(th, np.eye(n))
        assert _all_same(t1, t0), "whiten_t of the identity"
        out += list(t1)
    E = columns(n, 4)
    s0, s1 = f.sim_core(th, E), f.sim_grouped_core(th, E)          # th carries a mean: X mean + U^-1 E
    assert _same(s1, s0), "sim"
    out.append(s1)
    for fold in (None,) + tuple(folds):
        c0, c1 = f.cv_core(th, fold), f.cv_core(th, fold, grouped=True)
        assert _all_same(c1, c0), ("cv", None if fold is None else "folds")
        out += list(c1)
    return out


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_greedy_groups(n, m, cap):
    """the Bessel branch: blocks of 1 .. cap rows, the 64 / 65 seam; unwhiten and whiten_t of 1, 4, 5 and 9 columns with qdiag,
    at n <= 65 whiten_t of the identity, sim with a mean, leave-one-out"""
    th = problem(n)[2]
    assert np.any(th["mean"] != 0.0)
    f = _grouped_fit(n, m, cap)
    try:
        info = f.groups_info()
        _twins(f, th, n, identity=n <= 65)
    finally:
        f.close()
    _report("greedy groups: unwhiten, whiten_t, sim, leave-one-out", "n%d m%d cap%d blocks%d maxrows%d" % (n, m, cap, info["blocks"], info["maxrows"]))


def _fold_classes(n):
    """labels that hit every size class of the fold kernels, singles among them, scattered over the rows"""
    sizes = (5, 16, 17, 32, 33, 64, 65, 2)
    assert sum(sizes) < n
    lab = np.concatenate([np.full(s, k) for k, s in enumerate(sizes)] + [len(sizes) + np.arange(n - sum(sizes))])
    return np.random.default_rng(77).permutation(lab).astype(np.int32)


def test_fold_classes():
    n, m, cap = 300, 30, 64
    th = problem(n)[2]
    fold = _fold_classes(n)
    f = _grouped_fit(n, m, cap)
    try:
        assert f.r > 1
        c0, c1 = f.cv_core(th, fold, stats=True), f.cv_core(th, fold, stats=True, grouped=True)
        assert _same(c1[0], c0[0]) and _same(c1[1], c0[1]) and c1[2] == c0[2]
        assert c1[2]["singles"] == n - 234 and c1[2]["folds"] == 8 and c1[0].shape == (n, f.r)
    finally:
        f.close()
    _report("folds of 5 16 17 32 33 64 65 2 and singles, r > 1", "n%d m%d cap%d" % (n, m, cap))


def test_hand_made_partitions():
    import cocons_amd as ca
    from cocons_amd import host, workloads as wl
    # one block of 64 rows, all members: the last member writes 63 places and place m; 16 solves per wavefront
    n = 64
    locs, X, th, z = (a[:n] if i != 2 else a for i, a in enumerate(problem(65)[:4]))
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    try:
        info = f.set_groups(np.zeros(n, dtype=np.int32))
        assert (info["blocks"], info["maxrows"]) == (1, 64) and f.m == 63
        x0, x1 = f.unwhiten_core(th, np.eye(n)), f.unwhiten_grouped_core(th, np.eye(n))
        t0, t1 = f.whiten_t_core(th, np.eye(n)), f.whiten_t_grouped_core(th, np.eye(n))
        assert _same(x1, x0) and _all_same(t1, t0)
        assert np.all(t1[0][np.triu_indices(n)] != 0.0)               # U' is a full upper triangle: every place of every record
        c0, c1 = f.cv_core(th), f.cv_core(th, grouped=True)
        assert _all_same(c1, c0)
    finally:
        f.close()
    _report("one block of 64 member rows, the identity through U^-1 and U'", "n64")
    # a block of 64 rows whose only member is its last row, every other row a block of its own
    n = 300
    locs, th = problem(n)[0], problem(n)[2]
    nn = np.zeros((n, 63), dtype=np.int32, order="F")
    nn[:, :3] = host.vecchia_neighbours(locs, 3)
    nn[199] = host.vecchia_neighbours(locs[:200], 63)[199]
    f, wide, pl = _hand_fit(n, nn, np.arange(n, dtype=np.int32))
    try:
        assert pl["maxrows"] == 64 and pl["mask"][199] == 1 << 63 and pl["blocks"] == n
        _twins(f, th, n, cols=(5,))
    finally:
        f.close()
    _report("a block of 64 rows whose only member is the last, blocks of one row", "n%d" % n)
    # a block of 64 rows with 12 members: three solves per wavefront, all in one batch
    n = 65
    locs, th = problem(n)[0], problem(n)[2]
    nn = np.zeros((n, 63), dtype=np.int32, order="F")
    nn[:, :3] = host.vecchia_neighbours(locs, 3)
    nn[52:64] = VR.all_predecessors(64)[52:64]
    group = np.arange(n, dtype=np.int32)
    group[52:64] = 52
    f, wide, pl = _hand_fit(n, nn, group)
    try:
        b = pl["block"][52]
        assert pl["off"][b + 1] - pl["off"][b] == 64 and bin(pl["mask"][b]).count("1") == 12
        _twins(f, th, n, cols=(5,), identity=True)
    finally:
        f.close()
    _report("a block of 64 rows with 12 members", "n%d" % n)
    # the table padded to m = 63 while the plan's largest block is small: the record stride is wider than kb
    m, cap = 10, 17
    nn, group = tables(n, m, cap)[:2]
    locs, X, th, z = problem(n)[:4]
    wide = ca.vecchia_group_table(nn, group, 63)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    try:
        info = f.set_groups(group)
        assert f.m == 63 and info["maxrows"] <= cap < 64
        padded = _twins(f, th, n, cols=(5,), identity=True)
    finally:
        f.close()
    f = _grouped_fit(n, m, cap)
    try:
        assert f.m < 63
        assert _all_same(padded, _twins(f, th, n, cols=(5,), identity=True))      # the same model at the narrow stride
    finally:
        f.close()
    _report("a table padded to m = 63 over blocks of at most 17 rows", "n%d m%d cap%d" % (n, m, cap))


def test_n_fixed():
    """n_fixed in the middle of a block with members on both sides, n - 1, past the whole first blocks: the bits of sim_core,
    on one handle in a row -- the schedule of the n_fixed before does not leak -- and on fresh handles"""
    n, m, cap = 300, 10, 64
    th = problem(n)[2]
    group, wide = tables(n, m, cap)[1:]
    pl = GR.plan(wide, group)
    big = max(range(pl["blocks"]), key=lambda b: bin(pl["mask"][b]).count("1"))
    mem = [int(r) for q, r in enumerate(pl["rows"][pl["off"][big]:pl["off"][big + 1]]) if (pl["mask"][big] >> q) & 1]
    assert len(mem) >= 3
    mid = mem[len(mem) // 2]
    past = int(np.max(pl["rows"][:pl["off"][3]])) + 1                  # the first three blocks hold fixed rows only
    assert mem[0] < mid <= mem[-1] and 0 < past < n - 1
    seq = (mid, n - 1, past, 0, mid)
    fresh = {}
    for nf in set(seq):
        f = _grouped_fit(n, m, cap)
        try:
            fresh[nf] = f.sim_core(th, columns(n, 4)[nf:], n_fixed=nf, z_col=1)
        finally:
            f.close()
    f, g = _grouped_fit(n, m, cap), _grouped_fit(n, m, cap)
    try:
        for nf in seq:
            E = columns(n, 4)[nf:]
            got = f.sim_grouped_core(th, E, n_fixed=nf, z_col=1)
            assert got.shape == (n - nf, 4) and _same(got, fresh[nf]), nf
            assert _same(f.sim_core(th, E, n_fixed=nf, z_col=1), fresh[nf]), nf
            assert _same(g.sim_grouped_core(th, E, n_fixed=nf, z_col=1), fresh[nf]), nf       # grouped calls alone
    finally:
        f.close()
        g.close()
    _report("n_fixed in the middle of a block, n - 1, past the first blocks, 0; in a row on one handle", "n%d n_fixed %s" % (n, seq))


@pytest.mark.parametrize("nu", (0.5, 1.5, 2.5, None))
def test_the_four_modes(nu):
    n, m, cap = 300, 30, 64
    th0 = problem(n)[2]
    if nu is None:
        th, sl = th0, None
    else:
        th, sl = _theta(th0, smooth=np.zeros(3)), (nu, nu)
    f = _grouped_fit(n, m, cap, smooth_limits=sl)
    try:
        _twins(f, th, n, cols=(5,))
    finally:
        f.close()
    _report("modes", "nu %s n%d m%d cap%d" % ("free (Bessel)" if nu is None else "%.1f" % nu, n, m, cap))


# ---- failure ---------------------------------------------------------------------------------------------------------------------
def _raw(f, entry, th, n_fixed=0, fold=None):
    """(status, the outputs filled with 7 beforehand) of one of the eight entries, called through ctypes"""
    from cocons_amd import host
    n, r = f.n, f.r
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    W = np.asfortranarray(columns(n, 4))
    call = getattr(f._L, entry)
    if "unwhiten" in entry:
        out = np.full((n, 4), 7.0, order="F")
        return call(f._h, host._p(T), 4, host._p(W), host._p(out)), out
    if "sim" in entry:
        E = np.asfortranarray(W[n_fixed:])
        out = np.full((n - n_fixed, 4), 7.0, order="F")
        return call(f._h, host._p(T), host._p(mean), n_fixed, 0, 4, host._p(E), host._p(out)), out
    if "whiten_t" in entry:
        out, qd = np.full((n, 4), 7.0, order="F"), np.full(n, 7.0)
        return call(f._h, host._p(T), 4, host._p(W), host._p(out), host._p(qd)), out, qd
    resid, var = np.full((n, r), 7.0, order="F"), np.full(n, 7.0)
    st = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    lab = None if fold is None else np.ascontiguousarray(fold, dtype=np.int32)
    rc = call(f._h, host._p(T), host._p(mean), 0 if lab is None else int(lab.max()) + 1, None if lab is None else host._ip(lab),
              host._p(resid), host._p(var), st)
    return rc, resid, var, np.array(list(st), dtype=float)


TWINS = ("cocons_vecchia_unwhiten", "cocons_sim_vecchia", "cocons_vecchia_whiten_t", "cocons_cv_vecchia")


def _untouched(res):
    return all(np.all(a == 7.0) or np.all(a == -7.0) for a in res[1:])


def test_failing_block_in_the_middle_of_a_group():
    """the failing case of test_gpu_vecchia_group: the pivot of row 58 fails with the members 61 and 65 behind it in the block.
    Every grouped entry returns its twin's status, the outputs stay, and the handle is usable afterwards; with n_fixed past the
    failing member a later member of the block carries the status"""
    f, X, th0, z = _failing_fit(False)
    try:
        slope = np.array([0.0, 0.3, -0.2])
        up = float((X[57] - X[40]) @ slope) > 0
        good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
        before = _twins(f, good, 65, cols=(4,))
        for twin in TWINS:
            plain, grouped = _raw(f, twin, bad), _raw(f, twin + "_grouped", bad)
            assert plain[0] == 58 and grouped[0] == plain[0], twin
            assert _untouched(plain) and _untouched(grouped), twin
        codes = []
        for nf in (57, 58, 60, 61, 64):
            plain, grouped = _raw(f, "cocons_sim_vecchia", bad, n_fixed=nf), _raw(f, "cocons_sim_vecchia_grouped", bad, n_fixed=nf)
            assert grouped[0] == plain[0] and _untouched(grouped), nf
            codes.append(plain[0])
        assert codes[0] == 58 and codes[1] > 58 and codes[3] > codes[1]          # a later member carries the status
        after = _twins(f, good, 65, cols=(4,))                                   # the next calls on the handle are clean
        assert _all_same(before, after)
    finally:
        f.close()
    _report("failing block: the twin's status in every entry and with n_fixed 57 58 60 61 64 (%s)" % codes, "n65 row 58")


# ---- independence ----------------------------------------------------------------------------------------------------------------
def _with_env(name, value, call):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return call()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def test_bits_repeat_whatever_the_launch_order_the_fusion_and_the_calls_before():
    n, m, cap = 300, 10, 64
    th, Rz = problem(n)[2], problem(n)[7]
    fold = _fold_classes(n)
    E = columns(n, 4)

    def grouped(f):
        return [f.unwhiten_grouped_core(th, E), f.sim_grouped_core(th, E), f.sim_grouped_core(th, E[50:], n_fixed=50),
                *f.whiten_t_grouped_core(th, E), *f.cv_core(th, grouped=True), *f.cv_core(th, fold, grouped=True)]

    def plain(f):
        return [f.unwhiten_core(th, E), f.sim_core(th, E), f.sim_core(th, E[50:], n_fixed=50), *f.whiten_t_core(th, E),
                *f.cv_core(th), *f.cv_core(th, fold)]

    want = None
    for order in ("1", "0"):
        f = _with_order(order, lambda: _grouped_fit(n, m, cap))
        try:
            got = grouped(f)
            want = got if want is None else want
            assert _all_same(want, got), order
            assert _all_same(want, grouped(f)), order                                        # repeated
            assert _all_same(want, _with_env("COCONS_VECCHIA_SIM_FUSE", "0", lambda: grouped(f))), order
        finally:
            f.close()
    f = _grouped_fit(n, m, cap)
    try:
        assert _all_same(want, plain(f))                                                     # the twins on a fresh handle
    finally:
        f.close()
    # between the value, gradient, information and predict entries: every result at its fresh-handle bits
    lp, Xp = problem(n)[4], problem(n)[5]
    others = OrderedDict((("value", lambda f: f.neg2loglik_core(th, grouped=True)), ("whiten", lambda f: f.whiten_grouped_core(th, Rz)),
                          ("gradient", lambda f: f.neg2loglik_grad_core(th)[:4]),
                          ("grouped gradient", lambda f: f.neg2loglik_grad_core(th, grouped=True)[:4]),
                          ("information", lambda f: f.fisher_core(th, dirs19(3))),
                          ("grouped information", lambda f: f.fisher_core(th, dirs19(3), grouped=True)),
                          ("predict", lambda f: f.predict_knn_core(th, lp, Xp, 10))))

    def flat(out):
        return [np.asarray(o, dtype=float) for o in out if o is not None]

    want_other = {}
    for name, call in others.items():
        f = _grouped_fit(n, m, cap)
        try:
            want_other[name] = flat(call(f))                                                 # on a fresh handle
            assert _all_same(want, grouped(f)), name                                         # the grouped entries after it
        finally:
            f.close()
    f = _grouped_fit(n, m, cap)
    try:
        for k, (name, call) in enumerate(others.items()):
            got_new = grouped(f) if k % 2 == 0 else plain(f)                                 # grouped and ungrouped interleaved
            assert _all_same(want, got_new), name
            assert _all_same(want_other[name], flat(call(f))), name
        assert _all_same(want, grouped(f))
    finally:
        f.close()
    _report("repeats, both launch orders, COCONS_VECCHIA_SIM_FUSE=0, between value gradient information predict", "n%d m%d cap%d" % (n, m, cap))


# ---- refusals that need a handle ------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_handle():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n, m = 300, 10
    locs, X, th, z = problem(n)[:4]
    group, wide = tables(n, m, 64)[1:]
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    taper = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, 0.2)
    plain = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    try:
        for twin in TWINS:
            entry = twin + "_grouped"
            res = _raw(plain, entry, th)
            assert res[0] == -1 and _untouched(res), entry
            assert _lib.last_error().startswith(entry + ": the handle has no plan of grouped blocks"), _lib.last_error()
            for h in (dense, taper):
                res = _raw(h, entry, th)
                assert res[0] < 0 and _untouched(res), entry
                assert _lib.last_error().startswith(entry + ": not a Vecchia fit"), _lib.last_error()
        with pytest.raises(_lib.CoconsHipError, match="no plan"):
            plain.unwhiten_grouped_core(th, columns(n, 1))
        with pytest.raises(_lib.CoconsHipError, match="no plan"):
            plain.cv_core(th, grouped=True)
        ms3 = np.full(3, 7.0)
        T, W, out = host.theta_table(th), np.asfortranarray(columns(n, 1)), np.full((n, 1), 7.0, order="F")
        dbg = plain._L.cocons_debug_vecchia_sim_phases_grouped
        assert dbg(plain._h, host._p(T), 1, host._p(W), host._p(out), host._p(ms3)) == -1 and np.all(ms3 == 7.0) and np.all(out == 7.0)
        assert _lib.last_error().startswith("cocons_debug_vecchia_sim_phases_grouped: the handle has no plan")
        plain.set_groups(group)
        assert dbg(plain._h, host._p(T), 1, host._p(W), host._p(out), host._p(ms3)) == 0 and np.all(ms3 >= 0.0)
        assert _same(out, plain.unwhiten_core(th, W))
        # a fold above 128
        fold = np.zeros(n, dtype=np.int32)
        fold[129:] = 1
        for entry in ("cocons_cv_vecchia", "cocons_cv_vecchia_grouped"):
            res = _raw(plain, entry, th, fold=fold)
            assert res[0] == -1 and _untouched(res), entry
            assert _lib.last_error().startswith(entry + ": fold 0 holds 129 observations, more than the 128"), _lib.last_error()
        # z_col and n_fixed out of range
        mean, E = np.ascontiguousarray(th["mean"]), np.asfortranarray(columns(n, 4))
        so = np.full((n, 4), 7.0, order="F")
        for entry in ("cocons_sim_vecchia", "cocons_sim_vecchia_grouped"):
            call = getattr(plain._L, entry)
            assert call(plain._h, host._p(T), host._p(mean), 0, plain.r, 4, host._p(E), host._p(so)) == -1
            assert _lib.last_error() == entry + ": z_col = %d is outside 0 .. %d" % (plain.r, plain.r - 1)
            assert call(plain._h, host._p(T), host._p(mean), n, 0, 4, host._p(E), host._p(so)) == -1
            assert _lib.last_error() == entry + ": n_fixed = %d is outside 0 .. %d" % (n, n - 1)
        assert np.all(so == 7.0)
    finally:
        for h in (dense, taper, plain):
            h.close()
    _report("refusals: no plan, dense and taper handles, a fold of 129, z_col and n_fixed out of range", "n%d" % n)


def test_host_entries():
    """cocoSim_vecchia_grouped and cocoCV_vecchia_grouped on a borrowed handle give the ungrouped host entries' bits on it, and
    the same on a handle of their own"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m, cap = 300, 10, 64
    locs, X, th, z = problem(n)[:4]
    nn = tables(n, m, cap)[0]
    E = columns(n, 4)
    fold = _fold_classes(n)
    f = _grouped_fit(n, m, cap)
    try:
        s0 = ca.cocoSim_vecchia(th, locs, X, wl.SMOOTH_LIMITS, E, fit=f)
        s1 = ca.cocoSim_vecchia_grouped(th, locs, X, wl.SMOOTH_LIMITS, E, fit=f)
        c0 = ca.cocoCV_vecchia(th, locs, X, wl.SMOOTH_LIMITS, z, fold=fold, fit=f)
        c1 = ca.cocoCV_vecchia_grouped(th, locs, X, wl.SMOOTH_LIMITS, z, fold=fold, fit=f)
    finally:
        f.close()
    own_s = ca.cocoSim_vecchia_grouped(th, locs, X, wl.SMOOTH_LIMITS, E, nn=nn, max_rows=cap)
    own_c = ca.cocoCV_vecchia_grouped(th, locs, X, wl.SMOOTH_LIMITS, z, nn=nn, fold=fold, max_rows=cap)
    flat = lambda c: [np.asarray(v, dtype=float) for _, v in sorted(c.items())] if isinstance(c, dict) else [np.asarray(v, dtype=float) for v in c]  # noqa: E731
    assert _same(s1, s0) and _same(own_s, s0)
    assert _all_same(flat(c1), flat(c0)) and _all_same(flat(own_c), flat(c0))
    _report("host: cocoSim_vecchia_grouped, cocoCV_vecchia_grouped, borrowed and own handles", "n%d m%d cap%d" % (n, m, cap))
