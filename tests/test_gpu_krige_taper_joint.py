"""Joint prediction for tapered fits from the held band factor (cocons_krige_taper_joint) on the device:
against dense numpy algebra on the CPU oracle's entries, against cocons_krige_taper_apply (same bits), for bit-exactness
over repeats, ring depths, buffer layouts and the rows behind a request, for the output selection, the request that is not
positive definite, the refusals that need a handle, a state and a device memory the call leaves alone, and the R glue.

Cases (the generator is test_gpu_krige_taper._setup; Wendland-1 tapers of one delta for ref, pred and uu):
  A  n = 150,  delta 0.25, m = 700   six view tiles on a handle of nt = 2 tile columns with W = nt (no envelope to speak of);
                                     a partial 64-row strip and a partial 128 tile
  B  n = 900,  delta 0.15, m = 300   row 3 on top of an observation, row 4 without any neighbour
  C  n = 4000, delta 0.06, m = 300   W + D - 1 < nt: the deeper ring wraps
The error measure is max |difference| over the largest diagonal entry (cov), over max |draw| (sims) and over max |value|
(stochastic)."""
import functools

import numpy as np
import pytest

from test_gpu_krige_taper import _limits, _setup, _take_rows
from test_gpu_parity import _taper_pattern

pytestmark = pytest.mark.gpu

CASES = {"A": (150, 0.25, 700, False), "B": (900, 0.15, 300, True), "C": (4000, 0.06, 300, False)}

# Worst value per output over the three cases of test_matches_the_cpu_reference on MI355X (A / B / C):
#   cov         1.337e-15 / 5.234e-15 / 1.818e-15
#   sims        1.248e-14 / 3.883e-14 / 3.947e-14
#   stochastic  1.623e-14 / 4.799e-14 / 5.039e-14
# (diag(S_uu) - diag(cov) against apply's quadform: B 3.284e-15, C 1.123e-15.)  The bounds are 4 x the worst: what covers the
# spread between boxes and sum orders (the convention of test_gpu_krige_taper.py).  A measured value above 1e-10 would be a
# defect, not a bound.
MEASURED_WORST_COV = 5.234e-15
MEASURED_WORST_SIMS = 3.947e-14
MEASURED_WORST_STOCHASTIC = 5.039e-14
TOL_COV, TOL_SIMS, TOL_STOCHASTIC = 4 * MEASURED_WORST_COV, 4 * MEASURED_WORST_SIMS, 4 * MEASURED_WORST_STOCHASTIC


def _dense(pattern, entries, nrow, ncol):
    ci, rp = np.asarray(pattern[0]), np.asarray(pattern[1])
    A = np.zeros((nrow, ncol))
    A[np.repeat(np.arange(nrow), rp[1:] - rp[:-1]), ci - 1] = entries
    return A


@functools.lru_cache(maxsize=None)
def _case(name):
    """(setup, uu pattern, draws); shared, nothing below modifies it"""
    n, delta, m, special = CASES[name]
    s = _setup(n, delta, m, special)
    uu = _taper_pattern(s[6], delta)
    E = np.random.default_rng(70 + n).standard_normal((m, 3))
    return s, uu, E


@functools.lru_cache(maxsize=None)
def _reference(name, uu_scale=1.0):
    """Dense numpy algebra on the oracle's entries: (stochastic, S_uu, cov, mu).  S_uu from the lower triangle of the uu
    pattern, mirrored; uu_scale multiplies its off-diagonal taper entries."""
    from oracle import oracle as O
    O.build()
    s, uu, _ = _case(name)
    locs, X, th, _, z, ref_taper, lp, Xp, pt = s
    n, m = X.shape[0], Xp.shape[0]
    S = _dense(ref_taper, np.asarray(ref_taper[2]) * O.cov_rns_taper(th, locs, X, ref_taper[0], ref_taper[1], _limits()), n, n)
    C = _dense(pt, np.asarray(pt[2]) * O.cov_rns_taper_pred(th, locs, lp, X, Xp, pt[0], pt[1], _limits()), m, n)
    Su = np.tril(_dense(uu, _scaled(uu, uu_scale)[2] * O.cov_rns_taper(th, lp, Xp, uu[0], uu[1], _limits()), m, m))
    Su = Su + np.tril(Su, -1).T
    SiCt = np.linalg.solve(S, C.T)
    st = (z - X @ th["mean"]) @ SiCt
    cov = Su - C @ SiCt
    return st, Su, (cov + cov.T) / 2, Xp @ th["mean"] + st


def _scaled(uu, f):
    ci, rp, ent = uu
    rows = np.repeat(np.arange(len(rp) - 1), rp[1:] - rp[:-1])
    return ci, rp, np.where(ci - 1 == rows, ent, f * ent)


def _fit(s):
    import cocons_amd as ca
    locs, X, th, th2, z, ref_taper = s[:6]
    return ca.CoconsTaperFit(locs, X, z, _limits(), *ref_taper)


def _prepared(name):
    s, uu, E = _case(name)
    fit = _fit(s)
    fit.krige_taper_prepare(s[2])
    return fit, s, uu, E


def _eq(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def _default_depth(fit, m, monkeypatch):
    """the depth a call without COCONS_KRIGE_JOINT_DEPTH runs with, from the bytes of its ring against depth 1's (a ring slot
    is round_up(m, 64) x 128 doubles); nt - W + 1 when the ring stopped growing at nt slots"""
    monkeypatch.delenv("COCONS_KRIGE_JOINT_DEPTH", raising=False)
    b1 = fit.krige_taper_joint_bytes(m)
    monkeypatch.setenv("COCONS_KRIGE_JOINT_DEPTH", "1")
    b0 = fit.krige_taper_joint_bytes(m)
    monkeypatch.delenv("COCONS_KRIGE_JOINT_DEPTH")
    return 1 + (b1 - b0) // (8 * 128 * ((m + 63) // 64 * 64))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_matches_the_cpu_reference(name, monkeypatch):
    """stochastic, cov and three draws against the dense reference; the reference covariance is positive definite."""
    st_ref, Su, cov_ref, mu = _reference(name)
    ev = np.linalg.eigvalsh(cov_ref)
    assert ev.min() > 0
    fit, s, uu, E = _prepared(name)
    try:
        info = fit.krige_taper_info()
        m = CASES[name][2]
        if name == "A":
            assert info["nt"] == 2 and info["W"] == info["nt"] and (m + 127) // 128 == 6
        if name == "C":                  # the ring wraps; otherwise this case tests nothing
            D = _default_depth(fit, m, monkeypatch)
            print("krige_taper_joint case C: W = %d nt = %d default depth %d" % (info["W"], info["nt"], D))
            assert 1 <= D <= 16 and info["W"] + D - 1 < info["nt"], (info, D)
        st, cov, sims = fit.krige_taper_joint_core(s[6], s[7], s[8], uu, iiderrors=E)
    finally:
        fit.close()
    want = np.linalg.cholesky(cov_ref) @ E + mu[:, None]
    e_cov = float(np.max(np.abs(cov - cov_ref)) / np.max(np.diag(cov_ref)))
    e_sims = float(np.max(np.abs(sims - want)) / np.max(np.abs(want)))
    e_st = float(np.max(np.abs(st - st_ref)) / np.max(np.abs(st_ref)))
    print("krige_taper_joint vs reference %s: cov %.3e sims %.3e stochastic %.3e (eigenvalues %.3e .. %.3e)"
          % (name, e_cov, e_sims, e_st, ev.min(), ev.max()))
    assert np.array_equal(cov, cov.T)
    if name == "B":                      # row 4 has no neighbour: nothing is subtracted from its row and column of S_uu
        assert st[4] == 0.0
        assert np.array_equal(cov[4], Su_device_row(name, 4)) and np.array_equal(cov[:, 4], cov[4])
        assert np.count_nonzero(cov[4]) == 1 and cov[4, 4] > 0
    assert max(e_cov, e_sims, e_st) <= 1e-10, "a defect, not a bound"
    assert e_cov <= TOL_COV and e_sims <= TOL_SIMS and e_st <= TOL_STOCHASTIC, (e_cov, e_sims, e_st)


def Su_device_row(name, i):
    """Row i of S_uu as the device forms it: taper value times the device's own cov_rns_taper entry, columns <= i, and the
    mirror of column i below (case B's row 4 holds its diagonal only)."""
    import cocons_amd as ca
    s, uu, _ = _case(name)
    ci, rp, ent = uu
    m = len(rp) - 1
    vals = ent * ca.cov_rns_taper(s[2], s[6], s[7], ci, rp, _limits())
    D = np.tril(_dense(uu, vals, m, m))
    D = D + np.tril(D, -1).T
    return D[i]


@pytest.mark.parametrize("name", ["B", "C"])
def test_same_bits_as_apply(name):
    st_ref, Su, cov_ref, mu = _reference(name)
    fit, s, uu, E = _prepared(name)
    try:
        st0, qf0 = fit.krige_taper_core(s[6], s[7], s[8])
        st, cov, _ = fit.krige_taper_joint_core(s[6], s[7], s[8], uu)
    finally:
        fit.close()
    assert np.array_equal(st, st0)
    e = float(np.max(np.abs((np.diag(Su) - np.diag(cov)) - qf0)) / np.max(np.diag(cov_ref)))
    print("krige_taper_joint diag vs quadform %s: %.3e" % (name, e))
    assert e <= TOL_COV, e


def _leading(uu, k):
    """the uu pattern of the first k locations: rows < k, columns <= k"""
    ci, rp, ent = uu
    keep = np.concatenate([np.arange(rp[i] - 1, rp[i + 1] - 1)[ci[rp[i] - 1:rp[i + 1] - 1] <= k] for i in range(k)])
    cnt = [int(np.count_nonzero(ci[rp[i] - 1:rp[i + 1] - 1] <= k)) for i in range(k)]
    return ci[keep], np.concatenate([[1], 1 + np.cumsum(cnt)]).astype(np.int32), ent[keep]


def test_bit_exactness(monkeypatch):
    """Case C: repeats, the transpose, the ring depth (1, 3 and the default all wrap: W + 3 - 1 < nt), the buffer layout of the
    handle and the rows behind a request."""
    for k in ("COCONS_KRIGE_JOINT_DEPTH", "COCONS_TAPER_PACKED", "COCONS_TAPER_BAND"):
        monkeypatch.delenv(k, raising=False)
    fit, s, uu, E = _prepared("C")
    lp, Xp, pt = s[6], s[7], s[8]
    try:
        info = fit.krige_taper_info()
        assert info["W"] + 3 - 1 < info["nt"], info
        a = fit.krige_taper_joint_core(lp, Xp, pt, uu, iiderrors=E)
        assert _eq(a, fit.krige_taper_joint_core(lp, Xp, pt, uu, iiderrors=E))
        assert np.array_equal(a[1], a[1].T)
        for depth in ("1", "3"):
            monkeypatch.setenv("COCONS_KRIGE_JOINT_DEPTH", depth)
            b = fit.krige_taper_joint_core(lp, Xp, pt, uu)
            assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1]), depth
        monkeypatch.delenv("COCONS_KRIGE_JOINT_DEPTH")
        idx = np.arange(128)
        c = fit.krige_taper_joint_core(lp[:128], Xp[:128], _take_rows(pt, idx), _leading(uu, 128))
        assert np.array_equal(c[0], a[0][:128]) and np.array_equal(c[1], a[1][:128, :128])
    finally:
        fit.close()
    for env in ({"COCONS_TAPER_PACKED": "0"}, {"COCONS_TAPER_BAND": "0"}):
        for k in ("COCONS_TAPER_PACKED", "COCONS_TAPER_BAND"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        other = _fit(s)
        try:
            other.krige_taper_prepare(s[2])
            b = other.krige_taper_joint_core(lp, Xp, pt, uu)
        finally:
            other.close()
        assert np.array_equal(b[1], a[1]) and np.array_equal(b[0], a[0]), env


def test_depth_outside_its_range_is_refused(monkeypatch):
    from cocons_amd import _lib
    fit, s, uu, E = _prepared("B")
    try:
        for bad in ("0", "17", "-1", "four"):
            monkeypatch.setenv("COCONS_KRIGE_JOINT_DEPTH", bad)
            with pytest.raises(_lib.CoconsHipError, match="cocons_krige_taper_joint: COCONS_KRIGE_JOINT_DEPTH"):
                fit.krige_taper_joint_core(s[6], s[7], s[8], uu)
            with pytest.raises(_lib.CoconsHipError, match="cocons_krige_taper_joint_bytes: COCONS_KRIGE_JOINT_DEPTH"):
                fit.krige_taper_joint_bytes(300)
    finally:
        fit.close()


def test_output_selection():
    fit, s, uu, E = _prepared("B")
    lp, Xp, pt = s[6], s[7], s[8]
    try:
        full = fit.krige_taper_joint_core(lp, Xp, pt, uu, iiderrors=E)
        st1, none, sims1 = fit.krige_taper_joint_core(lp, Xp, pt, uu, iiderrors=E, cov=False)
        assert none is None and np.array_equal(sims1, full[2]) and np.array_equal(st1, full[0])
        st2, cov2, none = fit.krige_taper_joint_core(lp, Xp, pt, uu)
        assert none is None and np.array_equal(cov2, full[1]) and np.array_equal(st2, full[0])
        st3, none, none2 = fit.krige_taper_joint_core(lp, Xp, pt, uu, cov=False)
        assert none is None and none2 is None and np.array_equal(st3, full[0])
        # S_uu at other coordinates than the prediction's (stretched: a shift leaves every distance as it is): another
        # covariance, the same stochastic part
        st4, cov4, _ = fit.krige_taper_joint_core(lp, Xp, pt, uu, locs_unobs=1.01 * lp)
        assert np.array_equal(st4, full[0]) and not np.array_equal(cov4, full[1])
    finally:
        fit.close()


def _raw(fit, s, uu, nsim, E=None, **over):
    """the C entry with pre-filled outputs: (rc, message, stochastic, cov, sims)"""
    from cocons_amd import _lib
    dp, ip = (lambda a: a.ctypes.data_as(_lib.c_dp)), (lambda a: a.ctypes.data_as(_lib.ctypes.POINTER(_lib.c_int)))
    lp, Xp, pt = np.asfortranarray(s[6]), np.asfortranarray(s[7]), s[8]
    m = Xp.shape[0]
    ci, rp, te = (np.ascontiguousarray(a, dtype=t) for a, t in zip(pt, (np.int32, np.int32, np.float64)))
    cu, ru, tu = (np.ascontiguousarray(over.get(k, a), dtype=t)
                  for k, a, t in zip(("cu", "ru", "tu"), uu, (np.int32, np.int32, np.float64)))
    st, cov, sims = np.full(m, 7.0), np.full((m, m), 7.0, order="F"), np.full((m, max(nsim, 1)), 7.0, order="F")
    Ef = None if E is None else np.asfortranarray(E[:, :nsim])
    rc = fit._L.cocons_krige_taper_joint(fit._h, m, dp(lp), dp(Xp), ci.size, ip(ci), ip(rp), dp(te), None,
                                         over.get("nnz_uu", cu.size), ip(cu), ip(ru), dp(tu), dp(st), dp(cov), nsim,
                                         None if Ef is None else dp(Ef), dp(sims) if nsim else None)
    return rc, _lib.last_error(), st, cov, sims


def test_not_positive_definite():
    """Case B with every off-diagonal taper value of the uu pattern tripled: -5 with draws, success without."""
    import cocons_amd as ca
    import re
    cov_bad = _reference("B", 3.0)[2]
    assert np.linalg.eigvalsh(cov_bad).min() < 0
    fit, s, uu, E = _prepared("B")
    lp, Xp, pt = s[6], s[7], s[8]
    bad = _scaled(uu, 3.0)
    m = 300
    try:
        before = fit.krige_taper_core(lp, Xp, pt)
        rc, msg, st, cov, sims = _raw(fit, s, bad, 1, E)
        assert rc == -5, (rc, msg)
        assert msg.startswith("cocons_krige_taper_joint:") and "not positive definite" in msg, msg
        minor = int(re.search(r"leading minor (\d+) of", msg).group(1))
        print("krige_taper_joint not positive definite: minor %d" % minor)
        assert 1 <= minor <= m
        assert np.all(st == 7.0) and np.all(cov == 7.0) and np.all(sims == 7.0)
        with pytest.raises(ca.KrigeJointNotPositiveDefinite, match="leading minor"):
            fit.krige_taper_joint_core(lp, Xp, pt, bad, iiderrors=E[:, :1])
        st0, cov0, none = fit.krige_taper_joint_core(lp, Xp, pt, bad)
        assert none is None and np.max(np.abs(cov0 - cov_bad)) <= 1e-10 * np.max(np.diag(cov_bad))
        after = fit.krige_taper_core(lp, Xp, pt)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(st0, after[0])
    finally:
        fit.close()


def test_refusals_on_the_device():
    import cocons_amd as ca
    s, uu, E = _case("B")
    locs, X, th, _, z = s[:5]
    cu, ru, tu = uu
    m = 300
    who = "cocons_krige_taper_joint:"

    def refused(fit, what, **over):
        rc, msg, st, cov, sims = _raw(fit, s, uu, 1, E, **over)
        assert rc == -1 and msg.startswith(who) and what in msg, (rc, msg)
        assert np.all(st == 7.0) and np.all(cov == 7.0) and np.all(sims == 7.0)

    dense = ca.CoconsFit(locs, X, z, _limits())
    try:
        refused(dense, "not a taper fit")
    finally:
        dense.close()
    fit = _fit(s)
    try:
        refused(fit, "no kriging state")
        fit.krige_taper_prepare(th)
        # row 10 without its diagonal: the entry leaves, the later row pointers move up
        w = int(ru[10] - 1 + np.nonzero(cu[ru[10] - 1:ru[11] - 1] == 11)[0][0])
        r2 = ru.copy(); r2[11:] -= 1
        refused(fit, "row 11 does not hold its diagonal", cu=np.delete(cu, w), ru=r2, tu=np.delete(tu, w))
        row = int(np.nonzero(ru[1:] - ru[:-1] >= 2)[0][0])
        c3 = cu.copy(); c3[ru[row] - 1], c3[ru[row]] = cu[ru[row]], cu[ru[row] - 1]
        refused(fit, "not strictly increasing", cu=c3)
        r3 = ru.copy(); r3[m] += 1
        refused(fit, "rowpointers do not match nnz", ru=r3)
        c4 = cu.copy(); c4[0] = m + 1
        refused(fit, "column index out of range", cu=c4)
        assert fit.krige_taper_joint_core(s[6], s[7], s[8], uu)[1] is not None          # the handle still serves
        fit.krige_taper_release()
        refused(fit, "no kriging state")
    finally:
        fit.close()


def test_state_and_memory_are_left_alone():
    from test_gpu_krige import _free_bytes
    fit, s, uu, E = _prepared("C")
    lp, Xp, pt = s[6], s[7], s[8]
    m = CASES["C"][2]
    try:
        info = fit.krige_taper_info()
        st0, qf0 = fit.krige_taper_core(lp, Xp, pt)
        info = fit.krige_taper_info()                   # (the CSR staging of the state has seen this request)
        fit.krige_taper_joint_core(lp, Xp, pt, uu, iiderrors=E)       # the factorisation's scratch exists before the baseline
        _free_bytes()
        base = _free_bytes()
        fit.krige_taper_joint_core(lp, Xp, pt, uu, iiderrors=E)
        after = _free_bytes()
        assert abs(base - after) <= 64 * 2 ** 20, (base, after)
        assert fit.krige_taper_info() == info
        nbytes = fit.krige_taper_joint_bytes(m)
        mv, mpad = (m + 63) // 64 * 64, (m + 127) // 128 * 128
        npad = info["nt"] * 128
        assert 0 < nbytes < 8 * (mv * npad + mpad * mpad), (nbytes, info)       # no buffer of the full width
        assert fit.krige_taper_joint_bytes(m, nsim=3) == nbytes + 2 * 8 * (3 * m - 1)
        st1, qf1 = fit.krige_taper_core(lp, Xp, pt)
        assert np.array_equal(st0, st1) and np.array_equal(qf0, qf1)
    finally:
        fit.close()


def test_host_functions_against_the_reference():
    """cocoPredict_sparse_joint and cocoSim_cond_sparse_held on case B (own handles): the outputs of the core with the host
    lines around them."""
    import cocons_amd as ca
    st_ref, Su, cov_ref, mu = _reference("B")
    s, uu, E = _case("B")
    locs, X, th, _, z, ref_taper, lp, Xp, pt = s
    got = ca.cocoPredict_sparse_joint(th, locs, lp, X, Xp, _limits(), z, ref_taper, pt, uu)
    assert set(got) == {"systematic", "stochastic", "sd.pred", "cov.pred"}
    assert np.allclose(got["systematic"], Xp @ th["mean"], rtol=1e-13, atol=0)
    assert np.max(np.abs(got["cov.pred"] - cov_ref)) <= TOL_COV * np.max(np.diag(cov_ref))
    assert np.array_equal(got["sd.pred"], np.sqrt(np.diag(got["cov.pred"])))
    sims = ca.cocoSim_cond_sparse_held(th, locs, lp, np.column_stack([lp, np.arange(300.0)]), X, Xp, _limits(), z, ref_taper, pt,
                                       uu, E)
    want = np.linalg.cholesky(cov_ref) @ E + mu[:, None]
    assert sims.shape == (300, 3) and np.max(np.abs(sims - want)) <= TOL_SIMS * np.max(np.abs(want))


def test_glue_krige_taper_joint_matches_the_python_call():
    """`_cocons_hip_krige_taper_joint` through the R stub on case B: the bits of krige_taper_joint_core, with and without
    draws and cov; after release the glue reports the refusal."""
    from test_glue_exec import RStub
    R = RStub()
    s, uu, E = _case("B")
    locs, X, th, _, z, ref_taper, lp, Xp, pt = s
    fit = _fit(s)
    try:
        fit.krige_taper_prepare(th)
        want = fit.krige_taper_joint_core(lp, Xp, pt, uu, iiderrors=E)
    finally:
        fit.close()
    h = R.call("_cocons_hip_fit_create_taper", R.real(locs), R.real(X), R.real(z[:, None]), R.real(list(_limits())),
               R.integer([0]), R.integer(ref_taper[0]), R.integer(ref_taper[1]), R.real(ref_taper[2]))
    st = R.value(R.call("_cocons_hip_krige_taper_prepare", h, R.theta(th), R.real(th["mean"]), R.integer([1]), R.integer([0])))
    assert int(st[0][0]) == 0

    def taper(t):
        return R.plain_list([R.integer(t[0]), R.integer(t[1]), R.real(t[2])])

    rc, st, cov, sims = R.value(R.call("_cocons_hip_krige_taper_joint", h, R.real(lp), R.real(Xp), taper(pt), taper(uu), R.nil,
                                       R.real(E), R.integer([1])))
    assert int(rc[0]) == 0
    assert np.array_equal(st, want[0]) and np.array_equal(cov, want[1]) and np.array_equal(sims, want[2])
    rc, st, cov, sims = R.value(R.call("_cocons_hip_krige_taper_joint", h, R.real(lp), R.real(Xp), taper(pt), taper(uu), R.real(lp),
                                       R.nil, R.integer([1])))
    assert int(rc[0]) == 0 and sims is None and np.array_equal(cov, want[1])
    rc, st, cov, sims = R.value(R.call("_cocons_hip_krige_taper_joint", h, R.real(lp), R.real(Xp), taper(pt), taper(uu), R.nil,
                                       R.real(E), R.integer([0])))
    assert int(rc[0]) == 0 and cov is None and np.array_equal(sims, want[2])
    with pytest.raises(RuntimeError, match="uu_taper does not match"):
        R.call("_cocons_hip_krige_taper_joint", h, R.real(lp), R.real(Xp), taper(pt), taper((uu[0], uu[1][:-1], uu[2])), R.nil,
               R.nil, R.integer([1]))
    R.call("_cocons_hip_krige_taper_release", h)
    with pytest.raises(RuntimeError, match="cocons_krige_taper_joint"):
        R.call("_cocons_hip_krige_taper_joint", h, R.real(lp), R.real(Xp), taper(pt), taper(uu), R.nil, R.nil, R.integer([1]))
    R.L.stub_gc(0, None)
