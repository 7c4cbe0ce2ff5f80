"""U' and cross-validation on a Vecchia fit on the GPU (cocons_vecchia_transpose, cocons_vecchia_whiten_t, cocons_cv_vecchia)
against tests/vecchia_cv_reference.py on the oracle's matrices, on the problem of test_gpu_dense_sizes.problem and the tables
of test_gpu_vecchia.table and test_gpu_vecchia_sim.special.

Bound of every comparison with a reference: the project's parity bound, PARITY = 1e-8 of test_gpu_dense_sizes, relative to the
largest magnitude of the compared array.  (On these cases the reference in double differs from long double by at most
4.9e-14 -- tests/test_vecchia_cv_reference.py, five orders below the bound -- and cond(Q_BB) <= cond(Q) = cond(U)^2 <= 4096.)
Transposed lists are compared as integers, bits with np.array_equal.  Every test prints its worst error on one line that
starts with `vecchia-cv-report`; the measured figures stand in tests/golden/VECCHIA_CV_REPORT.md."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vecchia_reference as VR  # noqa: E402
import vecchia_cv_reference as VC  # noqa: E402
from test_gpu_dense_sizes import PARITY, problem  # noqa: E402
from test_gpu_vecchia import MS, SIZES, _duplicate_site, _fit, _theta, table  # noqa: E402
from test_gpu_vecchia_sim import special  # noqa: E402

pytestmark = pytest.mark.gpu

assert VC.SPECS[:len(SIZES) * len(MS)] == [(n, m) for n in SIZES for m in MS]


def _report(what, case, err):
    print("vecchia-cv-report gpu | %s | %s | %.2e" % (what, case, err))


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want)) / max(float(np.max(np.abs(want))), 1e-300))


@functools.lru_cache(maxsize=None)
def columns(n, c=3):
    W = np.asfortranarray(np.random.default_rng(1000 + n).standard_normal((n, c)))
    W.setflags(write=False)
    return W


def _case_fit(spec):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    c = VC.case(spec)
    return ca.CoconsVecchiaFit(c["locs"], c["X"], c["z"], wl.SMOOTH_LIMITS, c["nn"])


def _data_fit(nn, seed=5):
    """a handle over a table alone: no test that uses it evaluates a covariance"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = nn.shape[0]
    rng = np.random.default_rng(seed)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n), locs]))
    return ca.CoconsVecchiaFit(locs, X, rng.standard_normal(n), wl.SMOOTH_LIMITS, nn)


def _check_transpose(f, nn):
    ptr, rows = VC.transpose(nn)
    got = f.transpose()
    assert got["ptr"].dtype == np.int32 and got["rows"].dtype == np.int32
    assert np.array_equal(got["ptr"], ptr) and np.array_equal(got["rows"], rows)
    lens = np.diff(ptr)
    assert got["entries"] == rows.size == int(np.sum(np.asarray(nn) > 0))
    assert got["longest"] == int(lens.max()) and got["unnamed"] == int(np.sum(lens == 0))
    assert got["bytes"] >= 4 * (ptr.size + rows.size)
    again = f.transpose()
    assert np.array_equal(again["rows"], rows) and again["bytes"] == got["bytes"]
    return got


# ---- the transposed lists, exact integers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [s for s in VC.SPECS if s != "dup"], ids=str)
def test_transposed_lists_equal_the_reference_exactly(spec):
    nn = special(spec) if isinstance(spec, str) else table(*spec)
    f = _data_fit(nn)
    try:
        got = _check_transpose(f, nn)
    finally:
        f.close()
    if spec == "wide":
        assert got["longest"] == 578                # row 2 and the 577 late rows name row 1
    if spec == "zero":
        assert got["entries"] == 0 and got["unnamed"] == 641
    _report("transpose: ptr, rows, entries, longest, unnamed", str(spec), 0.0)


def _big_table(kind):
    n = 20000
    rng = np.random.default_rng(2020)
    if kind == "star":
        nn = np.zeros((n, 2), dtype=np.int32, order="F")
        nn[1:, 1] = 1
    elif kind == "random":
        nn = np.zeros((n, 3), dtype=np.int32, order="F")
        for t in range(3):
            nn[1:, t] = rng.integers(0, np.arange(1, n)) + 1            # any earlier row ..
        nn[np.arange(n) % 7 == 3, 1] = 0                                # .. with holes,
        dup = (nn[:, 0] == nn[:, 1]) | (nn[:, 0] == nn[:, 2]) | (nn[:, 1] == nn[:, 2])
        nn[dup, 1:] = 0                                                 # and no index twice in a row
    else:
        # lists of 63, 64, 65 (VECCHIA_T_WAVE = 64) and 4095, 4096, 4097 (VECCHIA_T_LDS = 4096) rows for the columns 1 .. 6,
        # their rows dealt out in a shuffled order; a second place names row 7 in every fifth row (a seventh list, 2499 rows)
        nn = np.zeros((n, 2), dtype=np.int32, order="F")
        lens = (63, 64, 65, 4095, 4096, 4097)
        who = rng.permutation(np.arange(7, n))[:sum(lens)]
        nn[who, 0] = np.repeat(np.arange(1, 7), lens)
        nn[np.arange(n) % 5 == 0, 1] = 7
        nn[:8, 1] = 0
    return nn


@pytest.mark.parametrize("kind", ("star", "random", "capacities"))
def test_transposed_lists_of_big_integer_tables(kind):
    """n = 20 000, no covariance evaluated.  star: one list of 19 999 rows (the sort in memory).  random: three places that
    name any earlier row.  capacities: list lengths on both sides of the sort's two capacity constants, VECCHIA_T_WAVE = 64
    (one wavefront, in registers) and VECCHIA_T_LDS = 4096 (one workgroup, in LDS): 63 / 64 / 65 and 4095 / 4096 / 4097."""
    nn = _big_table(kind)
    f = _data_fit(nn)
    try:
        got = _check_transpose(f, nn)
    finally:
        f.close()
    if kind == "star":
        assert got["longest"] == 19999 and got["unnamed"] == 19999
    if kind == "capacities":
        assert sorted(np.diff(got["ptr"])[:6]) == [63, 64, 65, 4095, 4096, 4097]
    _report("transpose, n = 20000", kind, 0.0)


# ---- U'W, diag(Q) and leave-one-out against the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("spec", VC.SPECS, ids=str)
def test_whiten_t_qdiag_and_leave_one_out(spec):
    c = VC.case(spec)
    n, th = c["nn"].shape[0], c["theta"]
    W = columns(n)
    want_ut, want_q = VC.whiten_t(c["U"], W)
    want_res, want_var = VC.loo(c["U"], c["R"])
    f = _case_fit(spec)
    try:
        ut, qd = f.whiten_t_core(th, W)
        ut1 = [f.whiten_t_core(th, W[:, k])[0] for k in range(3)]
        b = columns(n, 2)
        Ub = f.whiten_core(th, b)[0]
        adj = (np.sum(ut[:, :2] * b), np.sum(W[:, :2] * Ub), np.sum(np.abs(W[:, :2] * Ub)))
        resid, var, st = f.cv_core(th, stats=True)
    finally:
        f.close()
    errs = (_rel(ut, want_ut), _rel(qd, want_q), abs(adj[0] - adj[1]) / adj[2],
            _rel(resid, want_res), _rel(var, want_var))
    _report("whiten_t, qdiag, <U'w, b> = <w, U b>, loo resid, loo var", str(spec), max(errs))
    assert max(errs) < PARITY, errs
    assert resid.shape == c["R"].shape and st["singles"] == n and st["folds"] == 0
    for k in range(3):
        assert np.array_equal(ut1[k][:, 0], ut[:, k])              # the same bits for c = 1 and c = 3
    if n == 1:
        # nothing is left to predict from: the residual itself and Sigma_11
        assert _rel(resid, c["R"]) < PARITY and _rel(var, np.diag(c["S"])) < PARITY


# ---- folds against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", VC.FOLD_SPECS, ids=str)
def test_folds_of_every_size_class(spec):
    """fold sizes 2, 16, 17, 32, 33, 64, 65, 128 -- the seams of the four LDS classes -- with members scattered and in spatial
    blocks, labels that nobody carries, everybody else alone (n = 300 cannot hold the eight sizes, 357 observations, in one
    assignment: two assignments hold them between them, vecchia_cv_reference.layouts)"""
    c = VC.case(spec)
    n, th = c["nn"].shape[0], c["theta"]
    lays = VC.layouts(n, c["locs"])
    f = _case_fit(spec)
    try:
        got = {k: f.cv_core(th, fold, stats=True) for k, fold in lays.items()}
    finally:
        f.close()
    seen, worst = set(), 0.0
    for k, fold in lays.items():
        sizes = np.bincount(fold)
        assert np.sum(sizes == 0) > np.sum(sizes > 0)                    # most labels are carried by nobody
        seen |= set(int(s) for s in sizes if s > 1)
        want = VC.folds(c["U"], c["R"], fold, c["Q"])
        resid, var, st = got[k]
        assert st["singles"] == int(np.sum(sizes == 1)) and st["folds"] == int(np.sum(sizes > 1))
        errs = (_rel(resid, want[0]), _rel(var, want[1]))
        worst = max(worst, *errs)
        assert max(errs) < PARITY, (k, errs)
    assert seen == set(VC.FOLD_SIZES)
    _report("folds: resid, var over %s" % ", ".join(lays), str(spec), worst)


@pytest.mark.parametrize("spec", ((300, 10), (641, 30), "wide"), ids=str)
def test_folds_whose_members_share_no_row_and_folds_whose_members_name_each_other(spec):
    c = VC.case(spec)
    th = c["theta"]
    fold, (a, b), (p, d) = VC.pair_folds(c["nn"], c["Q"])
    assert c["Q"][a, b] == 0 and c["Q"][p, d] != 0
    want = VC.folds(c["U"], c["R"], fold, c["Q"])
    f = _case_fit(spec)
    try:
        resid, var = f.cv_core(th, fold)
        loo = f.cv_core(th)
    finally:
        f.close()
    errs = (_rel(resid, want[0]), _rel(var, want[1]))
    _report("folds of two: no shared row, one names the other", str(spec), max(errs))
    assert max(errs) < PARITY, errs
    # a diagonal Q_BB: the members' leave-one-out numbers (to rounding: the block's factorisation takes a square root)
    assert _rel(var[[a, b]], loo[1][[a, b]]) < 1e-14 and _rel(resid[[a, b]], loo[0][[a, b]]) < 1e-14


# ---- exactness ------------------------------------------------------------------------------------------------------------------
def test_exact_with_all_predecessors():
    """n = 64, m = 63, every predecessor: the Vecchia model is Sigma(theta), so leave-one-out and folds are cocons_cv_dense's"""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(6464)
    n = 64
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5]))
    th = wl.theta_full(scale0=np.log(0.2))
    th["mean"] = np.array([0.3, -0.15, 0.2])
    z = rng.standard_normal((n, 2))
    fold = (rng.permutation(n) % 5).astype(np.int32)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, VR.all_predecessors(n))
    d = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        errs = []
        for lab in (None, fold):
            got, want = f.cv_core(th, lab), d.cv_core(th, lab)
            errs += [_rel(got[0], want[0]), _rel(got[1], want[1])]
        host = ca.cocoCV_vecchia(th, locs, X, wl.SMOOTH_LIMITS, z, fold=fold * 10 + 3, fit=f)
        dense = ca.cocoCV_dense(th, locs, X, wl.SMOOTH_LIMITS, z, fold=fold, fit=d)
        last = f.cv_core(th, fold)
    finally:
        f.close()
        d.close()
    errs += [_rel(host[k], dense[k]) for k in ("mean.pred", "sd.pred", "resid")]
    _report("exact: cocons_cv_dense", "n64 m63", max(errs))
    assert max(errs) < PARITY, errs
    assert np.array_equal(host["resid"], last[0]) and np.array_equal(host["sd.pred"], np.sqrt(last[1]))


def test_host_function_makes_its_own_handle():
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    c = VC.case((300, 10))
    fold = VC.layouts(300, c["locs"])["blocks"]
    f = _case_fit((300, 10))
    try:
        want = f.cv_core(c["theta"], np.unique(fold, return_inverse=True)[1])
    finally:
        f.close()
    got = ca.cocoCV_vecchia(c["theta"], c["locs"], c["X"], wl.SMOOTH_LIMITS, c["z"], nn=c["nn"], fold=fold)
    knn = ca.cocoCV_vecchia(c["theta"], c["locs"], c["X"], wl.SMOOTH_LIMITS, c["z"], m=10, fold=fold)
    h = ca.CoconsVecchiaFit.from_knn(c["locs"], c["X"], c["z"], wl.SMOOTH_LIMITS, 10)
    try:
        want_knn = h.cv_core(c["theta"], np.unique(fold, return_inverse=True)[1])
    finally:
        h.close()
    assert np.array_equal(got["resid"], want[0]) and np.array_equal(got["sd.pred"], np.sqrt(want[1]))
    assert np.array_equal(got["mean.pred"], c["z"] - want[0])
    assert np.array_equal(knn["resid"], want_knn[0]) and np.array_equal(knn["sd.pred"], np.sqrt(want_knn[1]))
    with pytest.raises(ValueError, match="cocoCV_vecchia: give a neighbour table"):
        ca.cocoCV_vecchia(c["theta"], c["locs"], c["X"], wl.SMOOTH_LIMITS, c["z"])


# ---- bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ((641, 30), (300, 10), "wide"), ids=str)
def test_bits_repeat_and_a_fold_sees_its_members_alone(spec):
    c = VC.case(spec)
    n, th = c["nn"].shape[0], c["theta"]
    fold = VC.layouts(n, c["locs"])["blocks"] if not isinstance(spec, str) else VC.size_folds(n, (128, 33, 2), np.arange(n))
    sizes = np.bincount(fold)
    multi = np.nonzero(sizes[fold] > 1)[0]
    # the same folds of two or more under other labels, everybody else regrouped: pairs, in another order
    relab = np.zeros(n, dtype=np.int32)
    relab[multi] = (7 * n - 2 * fold[multi]).astype(np.int32)
    rest = np.nonzero(sizes[fold] == 1)[0][::-1]
    relab[rest] = 10 * n + np.arange(rest.size) // 2
    f, g = _case_fit(spec), _case_fit(spec)
    try:
        a, b = f.cv_core(th, fold), f.cv_core(th, fold)
        loo, loo2 = f.cv_core(th), f.cv_core(th)
        ones = f.cv_core(th, np.arange(n)[::-1].copy())
        other = g.cv_core(th, relab)                          # a handle that never saw the first assignment
    finally:
        f.close()
        g.close()
    for x, y in zip(a + loo, b + loo2):
        assert np.array_equal(x, y)
    assert np.array_equal(ones[0], loo[0]) and np.array_equal(ones[1], loo[1])          # folds of one are leave-one-out
    single = np.nonzero(sizes[fold] == 1)[0]
    assert np.array_equal(a[0][single], loo[0][single]) and np.array_equal(a[1][single], loo[1][single])
    assert np.array_equal(other[0][multi], a[0][multi]) and np.array_equal(other[1][multi], a[1][multi])
    _report("bits: repeat, folds of one, relabelled, regrouped", str(spec), 0.0)


def test_new_entries_between_the_others_keep_every_result_at_its_fresh_handle_bits():
    """value, whiten, unwhiten and the schedule share V->aos, V->B, V->W and the coefficients with the new entries"""
    n, m = 300, 30
    locs, X, th, z, lp, Xp, S, Rz = problem(n)
    W = columns(n)
    fold = VC.layouts(n, locs)["scattered"]

    def others(f):
        return [np.concatenate([[f.neg2loglik_core(th)[0]], f.neg2loglik_core(th)[1]]),
                np.concatenate([a.ravel() for a in f.whiten_core(th, Rz)]),
                f.unwhiten_core(th, W), f.schedule()["levels"], f.schedule(64)["levels"],
                np.concatenate([a.ravel() for a in f.neg2loglik_grad_core(th)[1:]])]

    def new(f):
        return [f.transpose()["rows"], *f.whiten_t_core(th, W), *f.cv_core(th), *f.cv_core(th, fold)]

    a, b, c = _fit(n, m), _fit(n, m), _fit(n, m)
    try:
        fresh_others, fresh_new = others(a), new(b)
        mixed_new = new(c)
        mixed_others = others(c)
        again_new = new(c)
        interleaved = []
        for k in range(6):
            interleaved.append(others(c)[k])
            c.cv_core(th, fold)
            c.whiten_t_core(th, W[:, :1])
    finally:
        for f in (a, b, c):
            f.close()
    for got in (mixed_new, again_new):
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh_new))
    for got in (mixed_others, interleaved):
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh_others))
    _report("order of calls", "n%d m%d" % (n, m), 0.0)


# ---- refusals that need a handle ------------------------------------------------------------------------------------------------
def _raw_cv(f, th, fold, nfold=None):
    from cocons_amd import host
    resid, var = np.full((f.n, f.r), 7.0, order="F"), np.full(f.n, 7.0)
    st = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    lab = None if fold is None else np.ascontiguousarray(fold, dtype=np.int32)
    nf = (0 if fold is None else int(lab.max()) + 1) if nfold is None else nfold
    rc = f._L.cocons_cv_vecchia(f._h, host._p(T), host._p(mean), nf, None if lab is None else host._ip(lab), host._p(resid),
                                host._p(var), st)
    return rc, resid, var, list(st)


def test_refusals_that_need_a_handle_and_the_bytes_of_the_handle():
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    n = 300
    locs, X, th, z = problem(n)[:4]
    T, mean = host.theta_table(th), np.ascontiguousarray(th["mean"])
    W, out, qd = np.asfortranarray(columns(n)), np.full((n, 3), 7.0, order="F"), np.full(n, 7.0)
    out4 = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    untouched = lambda r: np.all(r[1] == 7.0) and np.all(r[2] == 7.0) and r[3] == [-7] * 4      # noqa: E731
    vec = _fit(n, 10)
    dense = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    taper = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, 0.2)
    try:
        before = vec.info()["bytes"]
        fold = np.arange(n, dtype=np.int32)
        fold[:129] = 4                                                    # a fold of 129
        r = _raw_cv(vec, th, fold)
        assert r[0] == -1 and untouched(r)
        msg = _lib.last_error()
        assert msg.startswith("cocons_cv_vecchia: fold 4 holds 129 observations") and "cocons_vecchia_predict_knn" in msg
        assert vec.info()["bytes"] == before                              # refused before any device work
        fold[:] = 2                                                       # a fold that holds all n
        r = _raw_cv(vec, th, fold, nfold=5)
        assert r[0] == -1 and untouched(r)
        assert _lib.last_error() == "cocons_cv_vecchia: fold 2 holds all 300 observations"
        fold = np.arange(n, dtype=np.int32)
        for bad in (-1, n):
            fold[17] = bad
            r = _raw_cv(vec, th, fold, nfold=n)
            assert r[0] == -1 and untouched(r)
            assert _lib.last_error() == "cocons_cv_vecchia: label %d of observation 17 is outside [0, 300)" % bad
        fold[17] = 17
        fold[:128] = 0                                                    # 128 is served
        r = _raw_cv(vec, th, fold)
        assert r[0] == 0 and r[3][:2] == [n - 128, 1] and r[3][2] == vec.transpose()["entries"] and r[3][3] > 0
        # the other kinds of handle
        for kind, h in (("dense", dense), ("taper", taper)):
            L = vec._L
            assert L.cocons_vecchia_transpose(h._h, None, None, out4) == -1
            assert _lib.last_error().startswith("cocons_vecchia_transpose: not a Vecchia fit"), kind
            assert L.cocons_vecchia_whiten_t(h._h, host._p(T), 3, host._p(W), host._p(out), host._p(qd)) == -1
            assert _lib.last_error().startswith("cocons_vecchia_whiten_t: not a Vecchia fit"), kind
            r = _raw_cv(h, th, None)
            assert r[0] == -1 and untouched(r) and _lib.last_error().startswith("cocons_cv_vecchia: not a Vecchia fit"), kind
        assert np.all(out == 7.0) and np.all(qd == 7.0) and list(out4) == [-7] * 4
        # the lists and the coefficients are the handle's and are counted
        t = vec.transpose()
        assert vec.info()["bytes"] - before >= t["bytes"] + n * 11 * 8 and t["bytes"] >= 4 * (n + 1) + 5 * t["entries"]
    finally:
        vec.close()
        dense.close()
        taper.close()


def test_failing_block_returns_its_row_and_leaves_the_handle_usable():
    """test_gpu_vecchia's failing block (row 58 on the coordinates of row 41 and conditioned on it alone, the sign of the
    std.dev slopes decides its second pivot): a numerical refusal, not a device fault.  No test here is asked to produce -5."""
    import cocons_amd as ca
    from cocons_amd import _lib, host, workloads as wl
    locs, X, th0, z, nn = _duplicate_site(False)
    slope = np.array([0.0, 0.3, -0.2])
    up = float((X[57] - X[40]) @ slope) > 0
    good, bad = _theta(th0, std_dev=slope if up else -slope), _theta(th0, std_dev=-slope if up else slope)
    W = np.asfortranarray(columns(65))
    fold = (np.arange(65) // 4).astype(np.int32)
    f = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    g = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    try:
        fresh = g.cv_core(good, fold) + g.whiten_t_core(good, W)
        for lab in (None, fold):
            r = _raw_cv(f, bad, lab)
            assert r[0] == 58 and np.all(r[1] == 7.0) and np.all(r[2] == 7.0) and r[3] == [-7] * 4
        out, qd = np.full((65, 3), 7.0, order="F"), np.full(65, 7.0)
        assert f._L.cocons_vecchia_whiten_t(f._h, host._p(host.theta_table(bad)), 3, host._p(W), host._p(out), host._p(qd)) == 58
        assert np.all(out == 7.0) and np.all(qd == 7.0)
        with pytest.raises(_lib.CholeskyError) as e:
            f.cv_core(bad, fold)
        assert e.value.minor == 58
        again = f.cv_core(good, fold) + f.whiten_t_core(good, W)
        assert all(np.array_equal(x, y) for x, y in zip(again, fresh))
    finally:
        f.close()
        g.close()
    _report("failing block", "n65 row 58", 0.0)
