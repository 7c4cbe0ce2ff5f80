"""Kriging from a held factor (cocons_krige_prepare / _apply / _release / _info): cocoPredict's dense core at many new
locations from ONE factorisation of Sigma(theta).  Checked against the bordered path on the same handle (predict_core),
against the CPU oracle, for bit-identical rows whatever the chunking, for a state that the handle's other work leaves
alone, at full C5 size, for memory that does not grow with m, for refusals and recovery, and through the R glue."""
import threading
import time

import numpy as np
import pytest

from test_gpu_parity import _problem

pytestmark = pytest.mark.gpu

TOL = 1e-12          # against the bordered factorisation (another sum order) up to n = 1000; n = 4096 measured 4.4e-12


def _tol(n):
    return TOL if n <= 1000 else 1e-11


def _setup(n, seed, m):
    from cocons_amd import workloads as wl
    locs, X, th, rng = _problem(n, seed=seed)
    th["mean"] = np.array([0.3, -0.1, 0.2])
    z = rng.standard_normal(n)
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = wl.design_from_locs(lp)["std.covs"]
    return locs, X, th, z, lp, Xp


def _other_theta(th):
    th2 = {k: np.array(v, dtype=float) for k, v in th.items()}
    th2["scale"][0] += 0.3
    th2["std.dev"][1] -= 0.1
    th2["mean"] = np.array([-0.2, 0.1, 0.05])
    return th2


def _assert_close(got, want, tol=TOL):
    st, qf = got
    wst, wqf = want
    assert np.max(np.abs(st - wst)) <= tol * np.max(np.abs(wst)), np.max(np.abs(st - wst)) / np.max(np.abs(wst))
    assert np.max(np.abs(qf - wqf) / np.abs(wqf)) <= tol, np.max(np.abs(qf - wqf) / np.abs(wqf))


@pytest.mark.parametrize("n", [300, 1000, 4096])
def test_krige_matches_predict_core(n):
    """Same stochastic / quadform as the bordered factorisation on the same handle and theta; n = 300 and 1000 are not
    multiples of 128 (front padding), m = 1000 is not a multiple of max_rows = 192."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(n, 8000 + n, 1000)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    want = fit.predict_core(th, lp, Xp)
    fit.krige_prepare(th, max_rows=192)
    assert fit.krige_info() == {"prepared": True, "bytes": fit.krige_info()["bytes"], "rows": 192, "n": n}
    _assert_close(fit.krige_core(lp, Xp), want, _tol(n))
    fit.close()


def test_krige_chunked_vs_oracle(oracle):
    """cocoPredict_dense_chunked against oracle.cocoPredict_dense (LAPACK LU solve) on 256 rows at n = 2048, with the
    bounds of test_c5_predict_8192_vs_cpu."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(2048, 8100, 256)
    got = ca.cocoPredict_dense_chunked(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, max_rows=128)
    want = oracle.cocoPredict_dense(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z)
    scale = np.max(np.abs(want["stochastic"]))
    assert np.max(np.abs(got["stochastic"] - want["stochastic"])) <= 1e-8 * scale
    assert np.max(np.abs(got["systematic"] - want["systematic"])) <= 1e-13 * max(1.0, np.max(np.abs(want["systematic"])))
    assert np.max(np.abs(got["sd.pred"] - want["sd.pred"]) / want["sd.pred"]) <= 1e-8
    mean_only = ca.cocoPredict_dense_chunked(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, type="mean")
    assert set(mean_only) == {"systematic", "stochastic"}


def test_krige_chunking_and_repetition_change_nothing():
    """max_rows in {64, 1000, default} and a repeated apply: identical bits, row by row."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(1000, 8200, 1000)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    outs = []
    for mr in (64, 1000, 0):
        fit.krige_prepare(th, max_rows=mr)
        outs.append(fit.krige_core(lp, Xp))
        outs.append(fit.krige_core(lp, Xp))
    assert fit.krige_info()["rows"] >= 1000
    for st, qf in outs[1:]:
        assert np.array_equal(st, outs[0][0]) and np.array_equal(qf, outs[0][1])
    fit.close()


def test_krige_state_survives_other_work():
    """After prepare: an objective at another theta, predict_core at another theta with more rows (dA regrows) and a
    batch leave apply's output unchanged bit for bit; release + prepare at the other theta then matches predict_core."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(1000, 8300, 700)
    th2 = _other_theta(th)
    rng = np.random.default_rng(1)
    lp2 = rng.uniform(0, 1, size=(1500, 2))
    Xp2 = wl.design_from_locs(lp2)["std.covs"]
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th, max_rows=256)
    st0, qf0 = fit.krige_core(lp, Xp)
    fit.neg2loglik_core(th2)
    want2 = fit.predict_core(th2, lp2, Xp2)
    fit.neg2loglik_batch_core([th, th2, th])
    st1, qf1 = fit.krige_core(lp, Xp)
    assert np.array_equal(st0, st1) and np.array_equal(qf0, qf1)
    fit.krige_release()
    assert not fit.krige_info()["prepared"]
    fit.krige_prepare(th2)
    _assert_close(fit.krige_core(lp2, Xp2), want2)
    fit.close()


def test_krige_c5_properties_8192():
    """C5 at full size (n = m = 8192) predicting at the training locations: stochastic = residual, quadform = diag(Sigma)
    (the assertions of test_c5_predict_8192_properties)."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs = wl.grid_locs(128, 64)
    sc = wl.design_from_locs(locs)
    X = sc["std.covs"]
    th = wl.theta_full()
    th["mean"] = np.array([0.3, -0.1, 0.2])
    z = wl.synthetic_z(8192)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th)
    st, qf = fit.krige_core(locs, X)
    resid = z - X @ th["mean"]
    assert np.max(np.abs(st - resid)) < 1e-8 * np.max(np.abs(resid))
    diag = 1 / np.exp(-(X @ th["std.dev"])) + np.exp(X @ th["nugget"])
    assert np.max(np.abs(qf - diag)) < 1e-8 * np.max(diag)
    fit.close()


def _free_bytes():
    """Free device memory (hipMemGetInfo of the HIP runtime the library is linked against)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_krige_memory_does_not_grow_with_m():
    """n = 4096, m = 2000 then m = 200 000 (default chunk): the state's bytes and rows are the same, the free device
    memory never drops by more than those bytes (plus a margin) while the large apply runs, and every 97th row matches
    predict_core on those rows alone."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(4096, 8400, 200_000)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.neg2loglik_core(th)                         # the handle's own buffers exist before the baseline
    _free_bytes()
    base = _free_bytes()
    fit.krige_prepare(th)
    info_small = fit.krige_info()
    fit.krige_core(lp[:2000], Xp[:2000])
    assert fit.krige_info() == info_small
    low, done = [base], threading.Event()

    def sample():
        while not done.is_set():
            low[0] = min(low[0], _free_bytes())
            time.sleep(0.002)

    t = threading.Thread(target=sample)
    t.start()
    try:
        st, qf = fit.krige_core(lp, Xp)
    finally:
        done.set()
        t.join()
    info = fit.krige_info()
    assert info == info_small
    assert info["bytes"] <= 1.2 * 2 ** 30
    assert base - low[0] <= info["bytes"] + 64 * 2 ** 20, (base - low[0], info)
    idx = np.arange(0, 200_000, 97)
    _assert_close((st[idx], qf[idx]), fit.predict_core(th, lp[idx], Xp[idx]), _tol(4096))
    fit.close()


def test_krige_failure_refusals_and_nan_rows():
    """A Sigma with a mandatory non-positive pivot (fixed smoothness 1, no nugget: every entry the diagonal, minor 2):
    prepare reports the minor and leaves no state, so apply is refused; the handle then evaluates a good theta correctly.
    A taper handle is refused; NaN rows of X_pred give NaN in those rows only, the other rows keep their bits."""
    import cocons_amd as ca
    from cocons_amd import _lib
    from cocons_amd import workloads as wl
    from test_gpu_parity import _taper_pattern
    locs, X, th, z, lp, Xp = _setup(600, 8500, 300)
    bad = {k: np.zeros(3) for k in th}
    bad["scale"] = np.array([np.log(0.05), 0.0, 0.0])
    bad["nugget"] = np.array([-np.inf, 0.0, 0.0])
    good = th                                       # smooth != 0: the logistic branch, nu = 1, with a nugget
    fit = ca.CoconsFit(locs, X, z, (1.0, 1.0))
    with pytest.raises(_lib.CoconsHipError, match="cocons_krige_apply: no kriging state"):
        fit.krige_core(lp, Xp)                      # never prepared
    fit.krige_prepare(good)
    with pytest.raises(ca.CholeskyError) as ei:
        fit.krige_prepare(bad)
    assert ei.value.minor == 2
    assert not fit.krige_info()["prepared"]
    with pytest.raises(_lib.CoconsHipError, match="cocons_krige_apply"):
        fit.krige_core(lp, Xp)
    want = fit.predict_core(good, lp, Xp)
    fit.krige_prepare(good)
    _assert_close(fit.krige_core(lp, Xp), want)
    fit.close()

    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th, max_rows=128)
    st0, qf0 = fit.krige_core(lp, Xp)
    Xbad = Xp.copy()
    rows = [5, 130, 299]
    Xbad[rows, 1] = np.nan
    st1, qf1 = fit.krige_core(lp, Xbad)
    keep = np.setdiff1d(np.arange(300), rows)
    assert np.all(np.isnan(st1[rows])) and np.all(np.isnan(qf1[rows]))
    assert np.array_equal(st1[keep], st0[keep]) and np.array_equal(qf1[keep], qf0[keep])
    fit.close()

    ci, rp, ent = _taper_pattern(locs, 0.25)
    tf = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, ent)
    with pytest.raises(_lib.CoconsHipError, match="cocons_krige_prepare: not available on a taper fit"):
        tf.krige_prepare(th)
    tf.close()


def test_glue_krige_matches_krige_core():
    """`_cocons_hip_krige_prepare` / `_cocons_hip_krige` / `_cocons_hip_krige_release` through the R stub: bit for bit
    krige_core; after release the glue reports the refusal."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from test_glue_exec import RStub
    R = RStub()
    locs, X, th, z, lp, Xp = _setup(700, 8600, 500)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th, max_rows=192)
    want = fit.krige_core(lp, Xp)
    fit.close()
    h = R.call("_cocons_hip_fit_create", R.real(locs), R.real(X), R.real(z[:, None]), R.nil, R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]))
    st = R.value(R.call("_cocons_hip_krige_prepare", h, R.theta(th), R.real(th["mean"]), R.integer([1]), R.integer([192])))
    assert int(st[0][0]) == 0
    st, got = R.value(R.call("_cocons_hip_krige", h, R.real(lp), R.real(Xp)))
    assert int(st[0]) == 0 and got.shape == (500, 2)
    assert np.array_equal(got[:, 0], want[0]) and np.array_equal(got[:, 1], want[1])
    R.call("_cocons_hip_krige_release", h)
    with pytest.raises(RuntimeError, match="cocons_krige_apply"):
        R.call("_cocons_hip_krige", h, R.real(lp), R.real(Xp))
    R.L.stub_gc(0, None)
