"""Taper patterns on the device: cocons_taper_pattern against a numpy brute force over all pairs
(d = sqrt(dx dx + dy dy); row pointers and columns exactly, entries to 16 x 2^-52 relative), symmetry and repeatability,
the count call and the cap, cocons_krige_taper_apply_delta against cocons_krige_taper_apply fed with the exported pattern
(bit for bit) and with the numpy-built one (the bound between routes of test_gpu_krige_taper.py),
cocons_fit_create_taper_delta against cocons_fit_create_taper and the CPU oracle, and the R glue.

Every case first asserts on the CPU that no pair lies within 1e-12 delta of delta: membership is never a rounding question.
The reference entries are evaluated in the order of operations the header states (kernels.h pattern_taper_value), so a
device whose sqrt and division are correctly rounded gives the same doubles; the measured deviation is printed."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("wend1", "wend2", "sph")
ENTRY_RTOL = 16 * 2.0 ** -52
ROUTE_TOL = 4 * 1.912e-14            # tests/test_gpu_krige_taper.py: 4 x the measured worst difference between routes
N2LL_RTOL = 1e-8


def _taper(kind, h):
    u = 1.0 - h
    u2 = u * u
    if kind == "wend1":
        return (u2 * u2) * (4.0 * h + 1.0)
    if kind == "wend2":
        return ((u2 * u2) * u2) * (((35.0 * h) * h + 18.0 * h) + 3.0) / 3.0
    return (1.0 - 1.5 * h) + (0.5 * h) * (h * h)


def _brute(locs, q, delta, kind):
    """(colindices, rowpointers, entries) over all pairs, 1-based, and the distances' clearance from delta asserted"""
    q = locs if q is None else q
    dx = q[:, None, 0] - locs[None, :, 0]
    dy = q[:, None, 1] - locs[None, :, 1]
    d = np.sqrt(dx * dx + dy * dy)
    assert not np.any(np.abs(d - delta) <= 1e-12 * delta), "a pair sits on delta: choose another delta"
    mask = d <= delta
    rp = np.concatenate([[1], 1 + np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    ci = (np.nonzero(mask)[1] + 1).astype(np.int32)
    return ci, rp, _taper(kind, d[mask] / delta)


def _lattice_line(n, s):
    return np.column_stack([np.arange(n) * s, np.zeros(n)])


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (locs, queries, delta); built once, never modified"""
    rng = np.random.default_rng(42)
    s = 1.0 / 128
    line = _lattice_line(200, s)
    g = np.arange(20) * 0.05
    lattice = np.array([(x, y) for y in g for x in g])
    rnd = rng.uniform(0, 1, size=(300, 2))
    dup = np.vstack([rnd[:100], rnd[10:30], rnd[10:15]])
    inside = rng.uniform(0, 1, size=(40, 2))
    far = np.vstack([inside[:5], [[3.0, 0.5], [-2.0, -2.0]], inside[5:10], [[0.5, 1.4], [1.5, 1.5], [9.0, -9.0]]])
    # (the lattice spans [0, 0.95]^2: each of the first six lies 0.03 .. 0.043 off a lattice point of the box edge)
    near = np.array([[-0.03, 0.5], [0.98, 0.3], [0.6, -0.04], [0.2, 0.99], [-0.03, -0.03], [0.98, 0.98], [0.5, 0.5]])
    return {
        "n = 1": (np.array([[0.3, 0.7]]), np.array([[0.3, 0.7], [0.35, 0.75], [0.9, 0.1]]), 0.2),
        "m = 1": (rnd[:50], inside[:1], 0.3),
        "n = 700, delta larger than the domain": (rng.uniform(0, 1, size=(700, 2)), inside[:5], 3.0),
        "delta below the smallest spacing": (lattice, lattice[:50] + 0.025, 0.02),
        "collinear lattice, rows of 63": (line, None, 31.5 * s),
        "collinear lattice, rows of 65": (line, None, 32.5 * s),
        "collinear lattice, query rows of 64": (line, line[:150] + np.array([0.5 * s, 0.0]), 32.25 * s),
        "exact duplicates": (dup, inside[:10], 0.11),
        "a query on an observation": (rnd, np.vstack([inside[:3], rnd[17:18], inside[3:6], rnd[299:300]]), 0.08),
        "queries farther than delta outside the box": (rnd, far, 0.09),
        "queries within delta outside the box": (lattice, near, 0.07),
        "offset by 1e6": (1e6 + rng.uniform(0, 1, size=(400, 2)), 1e6 + rng.uniform(-0.05, 1.05, size=(60, 2)), 0.05),
    }


def _check(got, want, what):
    ci, rp, ent = got
    wci, wrp, went = want
    assert np.array_equal(rp, wrp), what
    assert np.array_equal(ci, wci), what
    dev = float(np.max(np.abs(ent - went) / np.abs(went))) if went.size and np.all(went != 0) else float(np.max(np.abs(ent - went), initial=0.0))
    print("pattern %s: nnz %d, largest entry deviation %.3e" % (what, ci.size, dev))
    assert np.all(np.abs(ent - went) <= ENTRY_RTOL * np.abs(went)), (what, dev)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(_cases()))
def test_pattern_against_brute_force(name, kind):
    import cocons_amd as ca
    locs, q, delta = _cases()[name]
    self_want = _brute(locs, None, delta, kind)
    _check(ca.taper_pattern(locs, delta, kind), self_want, name + " / self / " + kind)
    lens = np.diff(self_want[1])
    assert lens.min() >= 1                                   # every self row holds its diagonal
    if q is not None:
        want = _brute(locs, q, delta, kind)
        _check(ca.taper_pattern(locs, delta, kind, newlocs=q), want, name + " / query / " + kind)
        qlens = np.diff(want[1])
    # what the case is there for
    if name.startswith("n = 700"):
        assert np.all(lens == 700) and np.all(qlens == 700)
    elif name.startswith("delta below"):
        assert np.all(lens == 1) and np.all(qlens == 0)
    elif name.endswith("rows of 63"):
        assert lens.max() == 63
    elif name.endswith("rows of 65"):
        assert lens.max() == 65
    elif name.endswith("query rows of 64"):
        assert qlens.max() == 64
    elif name == "exact duplicates":
        assert np.sum(self_want[2] == 1.0) > locs.shape[0]  # d = 0 off the diagonal
    elif name == "a query on an observation":
        assert np.sum(want[2] == 1.0) == 2
    elif name.startswith("queries farther"):
        assert qlens[5] == 0 and qlens[6] == 0 and qlens[-1] == 0 and qlens[7] > 0
    elif name.startswith("queries within"):
        assert np.all(qlens[:6] > 0)


@pytest.mark.parametrize("name", ["exact duplicates", "n = 700, delta larger than the domain", "offset by 1e6",
                                  "collinear lattice, rows of 65"])
def test_symmetry_repeatability_count_and_cap(name):
    import cocons_amd as ca
    from cocons_amd import _lib
    L = _lib.load()
    locs, q, delta = _cases()[name]
    n = locs.shape[0]
    for kind in KINDS:
        ci, rp, ent = ca.taper_pattern(locs, delta, kind)
        ci2, rp2, ent2 = ca.taper_pattern(locs, delta, kind)
        assert np.array_equal(ci, ci2) and np.array_equal(rp, rp2) and np.array_equal(ent, ent2)
        # symmetric to the bit: the dense forms of pattern and entries
        A = np.zeros((n, n))
        P = np.zeros((n, n), dtype=bool)
        rows = np.repeat(np.arange(n), np.diff(rp))
        A[rows, ci - 1] = ent
        P[rows, ci - 1] = True
        assert np.array_equal(P, P.T) and np.array_equal(A, A.T) and np.all(np.diag(P)) and np.all(np.diag(A) == 1.0)
    # the count call alone, and a cap one short
    lf = np.asfortranarray(locs)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    nnz = ctypes.c_longlong(-1)
    rpc = np.full(n + 1, -7, dtype=np.int32)
    assert L.cocons_taper_pattern(n, dp(lf), n, None, delta, 1, 0, 0, ctypes.byref(nnz), ip(rpc), None, None) == 0
    assert nnz.value == ci.size and np.array_equal(rpc, rp)
    nnz2 = ctypes.c_longlong(-77)
    rpf, cif, entf = np.full(n + 1, -7, dtype=np.int32), np.full(ci.size, -7, dtype=np.int32), np.full(ci.size, -7.0)
    assert L.cocons_taper_pattern(n, dp(lf), n, None, delta, 1, 0, ci.size - 1, ctypes.byref(nnz2), ip(rpf), ip(cif),
                                  dp(entf)) == -1
    msg = _lib.last_error()
    assert msg.startswith("cocons_taper_pattern:") and str(ci.size) in msg, msg
    assert nnz2.value == -77 and np.all(rpf == -7) and np.all(cif == -7) and np.all(entf == -7.0)


# ---------------------------------------------------------------------------------------------------- kriging from delta
def _limits():
    from cocons_amd import workloads as wl
    return wl.SMOOTH_LIMITS


@functools.lru_cache(maxsize=None)
def _krige_setup(g):
    """A g x g lattice with its wend1 taper at 1.5 spacings (numpy), data, and 1000 new locations: inside, outside within
    and beyond delta, one on an observation.  Built once and shared; nothing modifies it."""
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(100 + g)
    n = g * g
    locs = wl.grid_locs(g)
    sp = 1.0 / (g - 1)
    assert abs(np.sort(np.unique(locs[:, 0]))[1] - sp) < 1e-12
    delta = 1.5 * sp
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full(scale0=np.log(0.15))
    th["mean"] = np.array([0.2, -0.1, 0.05])
    z = rng.standard_normal(n)
    m = 1000
    lp = rng.uniform(-0.04, 1.04, size=(m, 2))
    lp[3] = locs[n // 2]                     # on top of an observation
    lp[4] = np.array([4.0, 4.0])             # no neighbour
    lp[129] = np.array([-3.0, 0.5])          # the last row of the m = 130 request: empty too
    lp[999] = np.array([1.0 + 3 * sp, 1.0])
    Xp = np.column_stack([np.ones(m), rng.standard_normal(m), rng.standard_normal(m)])
    ref = _brute(locs, None, delta, "wend1")
    pred = _brute(locs, lp, delta, "wend1")
    return locs, X, th, z, delta, lp, Xp, ref, pred


def _rows(pt, m):
    ci, rp, ent = pt
    e = rp[m] - 1
    return ci[:e], rp[:m + 1], ent[:e]


LAYOUTS = {"default": {}, "no envelope": {"COCONS_TAPER_BAND": "0"}, "caller's order": {"COCONS_TAPER_RCM": "0"},
           "unpacked": {"COCONS_TAPER_PACKED": "0"}}


def _grid_bytes(locs, delta, nt):
    from cocons_amd import _lib
    L = _lib.load()
    lf = np.asfortranarray(locs)
    geom = np.zeros(5)
    assert L.cocons_debug_pattern_cells(lf.shape[0], lf.ctypes.data_as(_lib.c_dp), delta, 0, None, geom.ctypes.data_as(_lib.c_dp),
                                        None) == 0
    ncell, n = int(geom[3]) * int(geom[4]), lf.shape[0]
    return (2 * (ncell + 1) + n) * 4 + 2 * n * 8 + 3 * (nt + 1) * 4


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("g", [30, 10])
def test_apply_delta_equals_apply_bit_for_bit(g, layout, monkeypatch):
    import cocons_amd as ca
    locs, X, th, z, delta, lp, Xp, ref, pred = _krige_setup(g)
    for k in ("COCONS_TAPER_BAND", "COCONS_TAPER_RCM", "COCONS_TAPER_PACKED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    fit = ca.CoconsTaperFit(locs, X, z, _limits(), *ref)
    try:
        exported = ca.taper_pattern(locs, delta, "wend1", newlocs=lp)
        assert np.array_equal(exported[0], pred[0]) and np.array_equal(exported[1], pred[1])
        first = {}
        for max_rows in (64, 0):
            fit.krige_taper_prepare(th, max_rows=max_rows)
            info = fit.krige_taper_info()
            if g == 30 and layout == "default":
                assert 1 < info["W"] < info["nt"], info
            if g == 10:
                assert info["nt"] == 1
            grown = 0
            for m in (1, 130, 1000):
                pt = _rows(exported, m)
                want = fit.krige_taper_core(lp[:m], Xp[:m], pt)
                before = fit.krige_taper_info()["bytes"]
                got = fit.krige_taper_core_delta(lp[:m], Xp[:m], delta, "wend1")
                after = fit.krige_taper_info()["bytes"]
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (m, max_rows)
                assert fit.last_pattern_nnz == pt[0].size
                again = fit.krige_taper_core_delta(lp[:m], Xp[:m], delta, "wend1")
                assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
                assert fit.krige_taper_info()["bytes"] == after
                if after != before:
                    grown += 1
                    assert after - before == _grid_bytes(locs, delta, info["nt"])
                empty = np.nonzero(np.diff(pt[1]) == 0)[0]
                assert np.all(got[0][empty] == 0.0) and np.all(got[1][empty] == 0.0)
                if m >= 130:
                    assert {4, 129} <= set(empty.tolist())
                # max_rows does not enter the bits
                if m in first:
                    assert np.array_equal(got[0], first[m][0]) and np.array_equal(got[1], first[m][1])
                first[m] = got
            assert grown == 1                     # the grid, at the first call on each prepared state
    finally:
        fit.close()


def test_apply_delta_against_the_numpy_built_pattern_and_other_kinds():
    import cocons_amd as ca
    locs, X, th, z, delta, lp, Xp, ref, pred = _krige_setup(30)
    fit = ca.CoconsTaperFit(locs, X, z, _limits(), *ref)
    try:
        fit.krige_taper_prepare(th, max_rows=128)
        for kind in KINDS:
            host = _brute(locs, lp, delta, kind)
            want = fit.krige_taper_core(lp, Xp, host)
            got = fit.krige_taper_core_delta(lp, Xp, delta, kind)
            e = tuple(float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(got, want))
            print("apply_delta vs numpy-built pattern, %s: stochastic %.3e quadform %.3e" % (kind, e[0], e[1]))
            assert max(e) <= ROUTE_TOL, (kind, e)
        # the wrapper, against the chunked one fed with the numpy pattern
        a = ca.cocoPredict_sparse_delta(th, locs, lp, X, Xp, _limits(), z, ref, delta, "wend1", fit=fit, max_rows=128)
        b = ca.cocoPredict_sparse_chunked(th, locs, lp, X, Xp, _limits(), z, ref, pred, fit=fit, max_rows=128)
        for k in b:
            assert np.max(np.abs(a[k] - b[k])) <= ROUTE_TOL * np.max(np.abs(b[k])), k
    finally:
        fit.close()


def test_apply_delta_refusals_on_a_handle():
    import cocons_amd as ca
    locs, X, th, z, delta, lp, Xp, ref, pred = _krige_setup(10)
    fit = ca.CoconsTaperFit(locs, X, z, _limits(), *ref)
    dense = ca.CoconsFit(locs, X, z, _limits())
    try:
        with pytest.raises(ca.CoconsHipError, match="cocons_krige_taper_apply_delta: no kriging state"):
            fit.krige_taper_core_delta(lp[:5], Xp[:5], delta)
        with pytest.raises(ca.CoconsHipError, match="cocons_krige_taper_apply_delta: not a taper fit"):
            ca.CoconsTaperFit.krige_taper_core_delta(dense, lp[:5], Xp[:5], delta)
        fit.krige_taper_prepare(th)
        st, qf = fit.krige_taper_core_delta(lp[:0], Xp[:0], delta)
        assert st.size == 0 and fit.last_pattern_nnz == 0
    finally:
        fit.close()
        dense.close()


@pytest.mark.parametrize("n", [150, 700])
def test_create_taper_delta(oracle, n):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from test_gpu_parity import _problem
    locs, X, th, rng = _problem(n, seed=700 + n)
    z = rng.standard_normal((n, 1))
    delta = 0.25
    pp = wl.par_pos_full()
    tv = wl.theta_vector_from_lists(th, pp)
    lam = (0.0, 0.0, 0.0)
    for kind in KINDS:
        host = _brute(locs, None, delta, kind)
        exported = ca.taper_pattern(locs, delta, kind)
        a = ca.CoconsTaperFit.from_delta(locs, X, z, _limits(), delta, kind)
        b = ca.CoconsTaperFit(locs, X, z, _limits(), *exported)
        try:
            va, pa = a.neg2loglik_core(th)
            vb, pb = b.neg2loglik_core(th)
            assert va == vb and np.array_equal(pa, pb), kind
            got = ca.GetNeg2loglikelihoodTaper(tv, pp, exported, locs, X, _limits(), z, n, lam, fit=a)
            want = oracle.GetNeg2loglikelihoodTaper(tv, pp, host, locs, X, _limits(), z, n, lam)
            print("create_taper_delta n=%d %s: rel %.3e" % (n, kind, abs(got - want) / abs(want)))
            assert abs(got - want) <= N2LL_RTOL * abs(want), kind
        finally:
            a.close()
            b.close()


def test_glue_entries_return_what_the_python_calls_return():
    import cocons_amd as ca
    from test_glue_exec import RStub
    R = RStub()
    locs, X, th, z, delta, lp, Xp, ref, pred = _krige_setup(30)
    for kind, k in (("wend1", 1), ("sph", 3)):
        for q in (None, lp[:130]):
            want = ca.taper_pattern(locs, delta, kind, newlocs=q)
            got = R.value(R.call("_cocons_hip_taper_pattern", R.real(locs), R.nil if q is None else R.real(q), R.real([delta]),
                                 R.integer([k]), R.integer([0])))
            assert len(got) == 3
            for a, b in zip(got, want):
                assert np.array_equal(np.asarray(a).ravel(), b)
    ci, rp, ent = ref
    fit = ca.CoconsTaperFit(locs, X, z, _limits(), *ref)
    try:
        fit.krige_taper_prepare(th, max_rows=192)
        want = fit.krige_taper_core_delta(lp[:300], Xp[:300], delta, "wend2")
    finally:
        fit.close()
    h = R.call("_cocons_hip_fit_create_taper", R.real(locs), R.real(X), R.real(z[:, None]), R.real(list(_limits())),
               R.integer([0]), R.integer(ci), R.integer(rp), R.real(ent))
    st = R.value(R.call("_cocons_hip_krige_taper_prepare", h, R.theta(th), R.real(th["mean"]), R.integer([1]), R.integer([192])))
    assert int(st[0][0]) == 0
    args = (R.real(lp[:300]), R.real(Xp[:300]), R.real([delta]), R.integer([2]))
    st, got = R.value(R.call("_cocons_hip_krige_taper_delta", h, *args))
    assert int(st[0]) == 0 and got.shape == (300, 2)
    assert np.array_equal(got[:, 0], want[0]) and np.array_equal(got[:, 1], want[1])
    R.call("_cocons_hip_krige_taper_release", h)
    with pytest.raises(RuntimeError, match="cocons_krige_taper_apply_delta"):
        R.call("_cocons_hip_krige_taper_delta", h, *args)
    R.L.stub_gc(0, None)
