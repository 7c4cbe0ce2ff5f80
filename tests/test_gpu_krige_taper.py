"""Tapered kriging from a held band factor (cocons_krige_taper_prepare / _apply / _release / _info) on the
device: against the one-shot route cocons_predict_taper on the same handle, against the CPU oracle through
cocoPredict_sparse_chunked, bit-for-bit independence of the chunking and of the buffer layout, the state's survival of
the handle's other work, failures and refusals, memory that does not grow with m, and the R glue.

The error measure throughout is max |difference| / max |value| per output (quadform is 0 for rows without neighbours, so
no per-element relative error)."""
import functools
import threading
import time

import numpy as np
import pytest

from test_gpu_parity import _csr_within, _problem, _taper_pattern, _wendland1

pytestmark = pytest.mark.gpu

# Both device routes evaluate the same quantity to rounding, in different sum orders.  Measured worst difference between
# them over the three cases of test_matches_the_one_shot_route on MI355X: 1.912e-14 (stochastic at n = 900; n = 150:
# 8.4e-16, n = 4000: 1.77e-14; quadform at most 1.4e-15); the bound is 4 x that.  (The dense twin measures 4.4e-12 at
# n = 4096 and asserts 1e-11; a difference above 1e-10 would be a defect.)
MEASURED_WORST = 1.912e-14
ROUTE_TOL = 4 * MEASURED_WORST


def _limits():
    from cocons_amd import workloads as wl
    return wl.SMOOTH_LIMITS


def _pred_taper(lp, locs, delta):
    ci, rp = _csr_within(lp, locs, delta)
    ent = np.empty(ci.size)
    for i in range(lp.shape[0]):
        w0, w1 = rp[i] - 1, rp[i + 1] - 1
        d = np.sqrt(np.sum((locs[ci[w0:w1] - 1] - lp[i]) ** 2, axis=1))
        ent[w0:w1] = _wendland1(d, delta)
    return ci, rp, ent


def _take_rows(pt, idx):
    ci, rp, ent = pt
    cnt = (rp[1:] - rp[:-1])[idx]
    sel = np.concatenate([np.arange(rp[i] - 1, rp[i + 1] - 1) for i in idx]) if len(idx) else np.zeros(0, dtype=int)
    rp2 = np.concatenate([[1], 1 + np.cumsum(cnt)]).astype(np.int32)
    return ci[sel], rp2, ent[sel]


@functools.lru_cache(maxsize=None)
def _setup(n, delta, m, special=False):
    """Computed once per shape and shared (nothing below modifies it)."""
    locs, X, th, rng = _problem(n, seed=9000 + n)
    z = rng.standard_normal(n)
    ref_taper = _taper_pattern(locs, delta)
    lp = rng.uniform(0, 1, size=(m, 2))
    if special:
        lp[3] = locs[100]                    # on top of an observation
        lp[4] = np.array([4.0, 4.0])         # no neighbour: an empty row
    Xp = np.column_stack([np.ones(m), rng.standard_normal(m), rng.standard_normal(m)])
    pt = _pred_taper(lp, locs, delta)
    if special:
        assert pt[1][5] == pt[1][4]
    th2 = {k: np.array(v, dtype=float) for k, v in th.items()}
    th2["scale"] = th2["scale"] + np.array([0.15, 0.0, 0.0])
    th2["nugget"] = th2["nugget"] + np.array([0.2, 0.0, 0.0])
    return locs, X, th, th2, z, ref_taper, lp, Xp, pt


def _fit(s):
    import cocons_amd as ca
    locs, X, th, th2, z, ref_taper = s[:6]
    return ca.CoconsTaperFit(locs, X, z, _limits(), *ref_taper)


def _err(got, want):
    return tuple(float(np.max(np.abs(g - w)) / np.max(np.abs(w))) for g, w in zip(got, want))


def _assert_route(got, want, what):
    e = _err(got, want)
    print("krige_taper vs one-shot %s: stochastic %.3e quadform %.3e" % (what, e[0], e[1]))
    assert max(e) <= ROUTE_TOL, (what, e)


@pytest.mark.parametrize("n,delta,m,max_rows,special", [(150, 0.25, 100, 64, False), (900, 0.15, 300, 64, True),
                                                        (4000, 0.06, 1000, 192, False)])
def test_matches_the_one_shot_route(n, delta, m, max_rows, special):
    s = _setup(n, delta, m, special)
    th, lp, Xp, pt = s[2], s[6], s[7], s[8]
    fit = _fit(s)
    try:
        want = fit.predict_core(th, lp, Xp, pt)
        fit.krige_taper_prepare(th, max_rows=max_rows)
        info = fit.krige_taper_info()
        assert info["prepared"] and info["rows"] == max_rows and info["n"] == n and info["nt"] == (n + 127) // 128
        if n == 4000:
            assert info["W"] < info["nt"], info          # the ring wraps; otherwise this case tests nothing
        got = fit.krige_taper_core(lp, Xp, pt)
        _assert_route(got, want, "n=%d" % n)
        if special:
            assert got[0][4] == 0.0 and got[1][4] == 0.0
    finally:
        fit.close()


@pytest.mark.parametrize("type_", ["pred", "mean"])
def test_chunked_predict_vs_oracle(oracle, type_):
    """cocoPredict_sparse_chunked against the CPU restatement, with the bounds test_taper_predict_vs_oracle uses for the
    one-shot route."""
    import cocons_amd as ca
    s = _setup(900, 0.15, 300, True)
    locs, X, th, _, z, ref_taper, lp, Xp, pt = s
    got = ca.cocoPredict_sparse_chunked(th, locs, lp, X, Xp, _limits(), z, ref_taper, pt, type=type_, max_rows=128)
    want = oracle.cocoPredict_sparse(th, locs, lp, X, Xp, _limits(), z, ref_taper, pt)
    assert set(got) == ({"systematic", "stochastic", "sd.pred"} if type_ == "pred" else {"systematic", "stochastic"})
    assert np.allclose(got["systematic"], want["systematic"], rtol=1e-13, atol=0)
    scale = np.max(np.abs(want["stochastic"]))
    assert np.max(np.abs(got["stochastic"] - want["stochastic"])) < 1e-10 * scale
    assert got["stochastic"][4] == 0.0
    if type_ == "pred":
        assert np.max(np.abs(got["sd.pred"] - want["sd.pred"])) < 1e-9 * np.max(want["sd.pred"])


def test_chunking_repetition_and_block_permutation_are_bit_exact():
    s = _setup(4000, 0.06, 1000)
    th, lp, Xp, pt = s[2], s[6], s[7], s[8]
    fit = _fit(s)
    try:
        res = []
        for max_rows in (64, 448, 0):
            fit.krige_taper_prepare(th, max_rows=max_rows)
            a, b = fit.krige_taper_core(lp, Xp, pt), fit.krige_taper_core(lp, Xp, pt)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), max_rows
            res.append(a)
        for a in res[1:]:
            assert np.array_equal(a[0], res[0][0]) and np.array_equal(a[1], res[0][1])
        # the 15 whole 64-row blocks permuted (the last 40 rows stay): every row keeps its position modulo 64
        blocks = np.random.default_rng(5).permutation(15)
        idx = np.concatenate([np.arange(64 * b, 64 * b + 64) for b in blocks] + [np.arange(960, 1000)])
        assert not np.array_equal(idx, np.arange(1000))
        got = fit.krige_taper_core(lp[idx], Xp[idx], _take_rows(pt, idx))
        assert np.array_equal(got[0], res[0][0][idx]) and np.array_equal(got[1], res[0][1][idx])
    finally:
        fit.close()


def test_buffer_layouts_give_the_same_bits(monkeypatch):
    """COCONS_TAPER_PACKED=0 (the dense buffer, its band used) and COCONS_TAPER_BAND=0 (no envelope: hi[c] = nt and a
    ring of nt slots) against the default handle (packed band)."""
    s = _setup(3000, 0.07, 200)
    th, lp, Xp, pt = s[2], s[6], s[7], s[8]
    res = {}
    for name, env in (("default", {}), ("unpacked", {"COCONS_TAPER_PACKED": "0"}), ("noband", {"COCONS_TAPER_BAND": "0"})):
        for k in ("COCONS_TAPER_PACKED", "COCONS_TAPER_BAND"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        fit = _fit(s)
        try:
            fit.krige_taper_prepare(th, max_rows=128)
            info = fit.krige_taper_info()
            res[name] = fit.krige_taper_core(lp, Xp, pt)
            if name == "noband":
                assert info["W"] == info["nt"]
            else:
                assert info["W"] < info["nt"]
        finally:
            fit.close()
    for name in ("unpacked", "noband"):
        e = _err(res[name], res["default"])
        print("krige_taper layout %s vs default: stochastic %.3e quadform %.3e" % (name, e[0], e[1]))
    for name in ("unpacked", "noband"):
        assert np.array_equal(res[name][0], res["default"][0]) and np.array_equal(res[name][1], res["default"][1]), name


def test_state_survives_the_handles_other_work():
    s = _setup(900, 0.15, 300, True)
    th, th2, lp, Xp, pt = s[2], s[3], s[6], s[7], s[8]
    rng = np.random.default_rng(3)
    fit = _fit(s)
    try:
        small = np.arange(40)
        fit.predict_core(th, lp[small], Xp[small], _take_rows(pt, small))
        fit.krige_taper_prepare(th, max_rows=128)
        first = fit.krige_taper_core(lp, Xp, pt)
        info = fit.krige_taper_info()
        fit.neg2loglik_core(th2)
        fit.neg2loglik_grad_core(th2)
        fit.predict_core(th2, lp, Xp, pt)                      # more rows than before: the handle's buffer grows
        fit.neg2loglik_batch_core([th2, th, th2])
        fit.sim_core(th2, rng.standard_normal((900, 2)))
        again = fit.krige_taper_core(lp, Xp, pt)
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
        assert fit.krige_taper_info() == info
        fit.krige_taper_release()
        assert not fit.krige_taper_info()["prepared"] and fit.krige_taper_info()["bytes"] == 0
        fit.krige_taper_prepare(th2, max_rows=128)
        _assert_route(fit.krige_taper_core(lp, Xp, pt), fit.predict_core(th2, lp, Xp, pt), "other theta")
    finally:
        fit.close()


def test_failures_and_refusals():
    import cocons_amd as ca
    from cocons_amd import _lib
    s = _setup(900, 0.15, 300, True)
    locs, X, th, _, z, ref_taper, lp, Xp, pt = s
    ci, rp, ent = pt
    m = 300
    fit = _fit(s)
    try:
        with pytest.raises(_lib.CoconsHipError, match="cocons_krige_taper_apply: no kriging state"):
            fit.krige_taper_core(lp, Xp, pt)                   # never prepared
        fit.krige_taper_prepare(th, max_rows=128)
        bad = {k: np.array(v, dtype=float) for k, v in th.items()}
        bad["std.dev"][0] = -np.inf
        bad["nugget"][0] = -np.inf
        with pytest.raises(ca.CholeskyError):
            fit.krige_taper_prepare(bad)
        assert not fit.krige_taper_info()["prepared"]
        with pytest.raises(_lib.CoconsHipError, match="cocons_krige_taper_apply: no kriging state"):
            fit.krige_taper_core(lp, Xp, pt)
        want = fit.predict_core(th, lp, Xp, pt)
        fit.krige_taper_prepare(th, max_rows=128)
        st0, qf0 = fit.krige_taper_core(lp, Xp, pt)
        _assert_route((st0, qf0), want, "after a failed prepare")
        with pytest.raises(_lib.CoconsHipError, match="cocons_krige_taper_prepare: bad argument"):
            fit.krige_taper_prepare(th, z_col=1)               # z has one column; the state of the last prepare is kept
        with pytest.raises(_lib.CoconsHipError, match="cocons_krige_taper_prepare: bad argument"):
            fit.krige_taper_prepare(th, z_col=-1)
        # malformed CSR: -1, the message names the entry, the outputs are untouched
        L = fit._L
        dp, ip = (lambda a: a.ctypes.data_as(_lib.c_dp)), (lambda a: a.ctypes.data_as(_lib.ctypes.POINTER(_lib.c_int)))
        lpf, Xpf = np.asfortranarray(lp), np.asfortranarray(Xp)

        def raw(ci_, rp_, ent_, nnz=None, m_=m):
            st, qf = np.full(m, 7.0), np.full(m, 7.0)
            ci_, rp_ = np.ascontiguousarray(ci_, dtype=np.int32), np.ascontiguousarray(rp_, dtype=np.int32)
            rc = L.cocons_krige_taper_apply(fit._h, m_, dp(lpf), dp(Xpf), ci_.size if nnz is None else nnz, ip(ci_), ip(rp_),
                                            dp(ent_), dp(st), dp(qf))
            return rc, _lib.last_error(), st, qf

        row = int(np.nonzero(rp[1:] - rp[:-1] >= 2)[0][0])
        w = rp[row] - 1
        cases = {}
        cases["first pointer"] = (ci, rp - 1, ent)
        r2 = rp.copy(); r2[10] = r2[11] + 1
        cases["decreasing"] = (ci, r2, ent)
        r3 = rp.copy(); r3[m] += 1
        cases["last pointer"] = (ci, r3, ent)
        c1 = ci.copy(); c1[w] = 0
        cases["column 0"] = (c1, rp, ent)
        c2 = ci.copy(); c2[w] = 901
        cases["column n + 1"] = (c2, rp, ent)
        c3 = ci.copy(); c3[w], c3[w + 1] = ci[w + 1], ci[w]
        cases["unsorted"] = (c3, rp, ent)
        c4 = ci.copy(); c4[w + 1] = c4[w]
        cases["repeated"] = (c4, rp, ent)
        for name, args in cases.items():
            rc, msg, st, qf = raw(*args)
            assert rc == -1 and msg.startswith("cocons_krige_taper_apply:"), (name, rc, msg)
            assert np.all(st == 7.0) and np.all(qf == 7.0), name
        rc, msg, st, qf = raw(ci, rp, ent, m_=0)               # m = 0: nothing to do
        assert rc == 0 and np.all(st == 7.0)
        st_e, qf_e = fit.krige_taper_core(lp[:0], Xp[:0], (ci[:0], rp[:1], ent[:0]))
        assert st_e.size == 0 and qf_e.size == 0
        # NaN rows of X_pred: NaN in those rows only, the other rows keep their bits
        Xbad = Xp.copy()
        rows = [5, 130, 299]
        Xbad[rows, 1] = np.nan
        st1, qf1 = fit.krige_taper_core(lp, Xbad, pt)
        keep = np.setdiff1d(np.arange(m), rows)
        assert np.all(np.isnan(st1[rows])) and np.all(np.isnan(qf1[rows]))
        assert np.array_equal(st1[keep], st0[keep]) and np.array_equal(qf1[keep], qf0[keep])
    finally:
        fit.close()
    dense = ca.CoconsFit(locs, X, z, _limits())
    try:
        T = ca.host.theta_table(th)
        mean = np.ascontiguousarray(th["mean"], dtype=np.float64)
        assert dense._L.cocons_krige_taper_prepare(dense._h, dp(T), dp(mean), 0, 0) == -1
        assert _lib.last_error().startswith("cocons_krige_taper_prepare: not a taper fit")
        st, qf = np.full(m, 7.0), np.full(m, 7.0)
        assert dense._L.cocons_krige_taper_apply(dense._h, m, dp(lpf), dp(Xpf), ci.size, ip(ci), ip(rp), dp(ent), dp(st),
                                                 dp(qf)) == -1
        assert _lib.last_error().startswith("cocons_krige_taper_apply: not a taper fit")
        assert np.all(st == 7.0) and np.all(qf == 7.0)
    finally:
        dense.close()


def test_memory_does_not_grow_with_m():
    """n = 4000, m = 20 000 in chunks of 1024: the state's info is the same before and after, the free device memory never
    drops by more than the reported bytes (plus a margin) while the apply runs, and every 97th row matches predict_core
    on those rows alone."""
    from test_gpu_krige import _free_bytes
    s = _setup(4000, 0.06, 20000)
    th, lp, Xp, pt = s[2], s[6], s[7], s[8]
    fit = _fit(s)
    try:
        fit.neg2loglik_core(th)                         # the handle's own buffers exist before the baseline
        _free_bytes()
        base = _free_bytes()
        fit.krige_taper_prepare(th, max_rows=1024)
        before = fit.krige_taper_info()
        low, done = [base], threading.Event()

        def sample():
            while not done.is_set():
                low[0] = min(low[0], _free_bytes())
                time.sleep(0.002)

        t = threading.Thread(target=sample)
        t.start()
        try:
            st, qf = fit.krige_taper_core(lp, Xp, pt)
        finally:
            done.set()
            t.join()
        info = fit.krige_taper_info()
        assert info == before and info["rows"] == 1024
        assert base - low[0] <= info["bytes"] + 64 * 2 ** 20, (base - low[0], info)
        idx = np.arange(0, 20000, 97)
        _assert_route((st[idx], qf[idx]), fit.predict_core(th, lp[idx], Xp[idx], _take_rows(pt, idx)), "every 97th row")
    finally:
        fit.close()


def test_glue_krige_taper_matches_krige_taper_core():
    """`_cocons_hip_krige_taper_prepare` / `_cocons_hip_krige_taper` / `_cocons_hip_krige_taper_release` through the R stub:
    bit for bit krige_taper_core; after release the glue reports the refusal."""
    from test_glue_exec import RStub
    R = RStub()
    s = _setup(900, 0.15, 300, True)
    locs, X, th, _, z, ref_taper, lp, Xp, pt = s
    ci, rp, ent = ref_taper
    fit = _fit(s)
    try:
        fit.krige_taper_prepare(th, max_rows=192)
        want = fit.krige_taper_core(lp, Xp, pt)
    finally:
        fit.close()
    h = R.call("_cocons_hip_fit_create_taper", R.real(locs), R.real(X), R.real(z[:, None]), R.real(list(_limits())),
               R.integer([0]), R.integer(ci), R.integer(rp), R.real(ent))
    st = R.value(R.call("_cocons_hip_krige_taper_prepare", h, R.theta(th), R.real(th["mean"]), R.integer([1]), R.integer([192])))
    assert int(st[0][0]) == 0
    args = (R.real(lp), R.real(Xp), R.integer(pt[0]), R.integer(pt[1]), R.real(pt[2]))
    st, got = R.value(R.call("_cocons_hip_krige_taper", h, *args))
    assert int(st[0]) == 0 and got.shape == (300, 2)
    assert np.array_equal(got[:, 0], want[0]) and np.array_equal(got[:, 1], want[1])
    R.call("_cocons_hip_krige_taper_release", h)
    with pytest.raises(RuntimeError, match="cocons_krige_taper_apply"):
        R.call("_cocons_hip_krige_taper", h, *args)
    R.L.stub_gc(0, None)
