"""Joint prediction from the held factor (cocons_krige_joint): the predictive covariance between new locations and the
conditional draws, against the joint factorisation on the same handle (cocons_sim_cond_dense), against the CPU oracle,
against krige_core, for determinism, for a state and a device memory the call leaves alone, for the request that is not
positive definite, and through the R glue.

Shapes: n = 300 gives npad = 384 with 84 rows of front padding; m = 200 a partial 64-row strip and a partial 128 tile;
m = 300 three tile rows of the covariance (diagonal, off-diagonal and partial tiles); m = 130 a V whose 192 rows end before
the covariance's 256 do."""
import numpy as np
import pytest

import krige_joint_reference as ref
from test_gpu_krige import TOL, _free_bytes, _setup

pytestmark = pytest.mark.gpu


def _p(a):
    from cocons_amd import _lib
    return a.ctypes.data_as(_lib.c_dp)


@pytest.mark.parametrize("n,m", [(300, 200), (1000, 300)])
def test_joint_matches_the_joint_factorisation(n, m):
    """Same handle, same draws: sims against sim_cond_core within 1e-10 of max |want| (the project's 1e-12 between two sum
    orders of the solve, times the ~50 by which the Cholesky of the predictive covariance amplifies a perturbation of it,
    rounded up), cov against L L' within 1e-12 of max diag (TOL), L = the lower triangle of sim_cond_core(E = I) - mu with
    mu the trend sim_cond_core itself adds (its column for E = 0).
    Measured: (300, 200) sims 8.9e-14, cov 5.0e-15; (1000, 300) sims 5.9e-13, cov 2.5e-14."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(n, 9000 + n, m)
    E = np.random.default_rng(n).standard_normal((m, 3))
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    want = fit.sim_cond_core(th, lp, Xp, lp, E)
    unit = fit.sim_cond_core(th, lp, Xp, lp, np.hstack([np.eye(m), np.zeros((m, 1))]))
    fit.krige_prepare(th)
    st, cov, sims = fit.krige_joint_core(lp, Xp, iiderrors=E)
    fit.close()
    d_sims = np.max(np.abs(sims - want)) / np.max(np.abs(want))
    mu = unit[:, m]
    assert np.max(np.abs(mu - (Xp @ th["mean"] + st))) <= TOL * np.max(np.abs(mu))
    L = np.tril(unit[:, :m] - mu[:, None])
    d_cov = np.max(np.abs(cov - L @ L.T)) / np.max(np.diag(cov))
    print("n = %d m = %d: sims %.2e  cov %.2e" % (n, m, d_sims, d_cov))
    assert d_sims <= 1e-10, d_sims
    assert d_cov <= TOL, d_cov


def test_joint_more_new_locations_than_observations():
    """n = 300, m = 700: more rows than the handle has observations, and a covariance of six tiles -- from five tiles on the
    factorisation of the view runs on the engine schedule.  Bounds and references of the test above.
    Measured: sims 2.3e-13, cov 1.1e-14."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m = 300, 700
    locs, X, th, z, lp, Xp = _setup(n, 9050, m)
    E = np.random.default_rng(n).standard_normal((m, 3))
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    unit = fit.sim_cond_core(th, lp, Xp, lp, np.hstack([np.eye(m), E, np.zeros((m, 1))]))
    fit.krige_prepare(th)
    st, cov, sims = fit.krige_joint_core(lp, Xp, iiderrors=E)
    fit.close()
    want, mu = unit[:, m:m + 3], unit[:, m + 3]
    d_sims = np.max(np.abs(sims - want)) / np.max(np.abs(want))
    L = np.tril(unit[:, :m] - mu[:, None])
    d_cov = np.max(np.abs(cov - L @ L.T)) / np.max(np.diag(cov))
    print("n = %d m = %d: sims %.2e  cov %.2e" % (n, m, d_sims, d_cov))
    assert np.array_equal(cov, cov.T)
    assert d_sims <= 1e-10, d_sims
    assert d_cov <= TOL, d_cov


@pytest.fixture(scope="module")
def oracle_problem(oracle):
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(1000, 9100, 300)
    newdataset = np.column_stack([lp + 0.01, np.arange(300.0)])
    return locs, X, th, z, lp, Xp, newdataset


def test_joint_against_oracle(oracle, oracle_problem):
    """n = 1000, m = 300: cocoPredict_dense_joint's cov.pred against the numpy restatement (within 1e-8 of max diag) and
    cocoSim_cond_dense_held against oracle.cocoSim_cond_dense (within 1e-8 of max |want|) with Sigma_uu taken at the new
    locations shifted by 0.01 -- the second coordinate set.  1e-8 is the project's parity bound.
    Measured: cov.pred 3.2e-14, sd.pred 3.1e-13, draws 9.7e-13."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp, newdataset = oracle_problem
    got = ca.cocoPredict_dense_joint(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z)
    assert set(got) == {"systematic", "stochastic", "sd.pred", "cov.pred"}
    S, C, Suu = ref.matrices(oracle, th, locs, X, lp, Xp, lp, wl.SMOOTH_LIMITS)
    want = ref.cov_lu(S, C, Suu)
    d_cov = np.max(np.abs(got["cov.pred"] - want)) / np.max(np.diag(want))
    pred = oracle.cocoPredict_dense(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z)
    d_sd = np.max(np.abs(got["sd.pred"] - pred["sd.pred"]) / pred["sd.pred"])
    assert np.max(np.abs(got["stochastic"] - pred["stochastic"])) <= 1e-8 * np.max(np.abs(pred["stochastic"]))
    E = np.random.default_rng(11).standard_normal((300, 3))
    sims = ca.cocoSim_cond_dense_held(th, locs, lp, newdataset, X, Xp, wl.SMOOTH_LIMITS, z, E)
    wsim = oracle.cocoSim_cond_dense(th, locs, lp, newdataset, X, Xp, wl.SMOOTH_LIMITS, z, E)
    d_sim = np.max(np.abs(sims - wsim)) / np.max(np.abs(wsim))
    print("oracle: cov.pred %.2e  sd.pred %.2e  draws %.2e" % (d_cov, d_sd, d_sim))
    assert d_cov <= 1e-8 and d_sd <= 1e-8 and d_sim <= 1e-8


def test_joint_is_consistent_with_krige_core():
    """stochastic: the bits of krige_core; diag(cov) = diag(Sigma_uu) - quadform within 1e-12 of the diagonal; cov equals its
    transpose bit for bit."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(300, 9200, 200)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th, max_rows=64)
    st0, qf0 = fit.krige_core(lp, Xp)
    st, cov, sims = fit.krige_joint_core(lp, Xp)
    fit.close()
    assert sims is None
    assert np.array_equal(st, st0)
    diag = 1 / np.exp(-(Xp @ th["std.dev"])) + np.exp(Xp @ th["nugget"])
    assert np.max(np.abs(np.diag(cov) - (diag - qf0)) / diag) <= 1e-12
    assert np.array_equal(cov, cov.T)


def test_joint_is_deterministic():
    """m = 300 on n = 300: two calls agree bit for bit; the request of the first 130 rows equals the leading 130 x 130 block
    and the first 130 entries; cov = None leaves the draws, nsim = 0 leaves cov."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(300, 9300, 300)
    E = np.random.default_rng(3).standard_normal((300, 2))
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th)
    a = fit.krige_joint_core(lp, Xp, iiderrors=E)
    b = fit.krige_joint_core(lp, Xp, iiderrors=E)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    st1, cov1, _ = fit.krige_joint_core(lp[:130], Xp[:130])
    assert np.array_equal(st1, a[0][:130]) and np.array_equal(cov1, a[1][:130, :130])
    st2, none, sims2 = fit.krige_joint_core(lp, Xp, iiderrors=E, cov=False)
    assert none is None and np.array_equal(sims2, a[2]) and np.array_equal(st2, a[0])
    st3, cov3, none = fit.krige_joint_core(lp, Xp)
    assert none is None and np.array_equal(cov3, a[1]) and np.array_equal(st3, a[0])
    fit.close()


def test_joint_leaves_state_and_memory_alone():
    """krige_info() reads the same before and after, a later krige_core returns the bits it returned before, and the free
    device memory after the call is within 64 MiB of its value before (everything the call allocates is released)."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z, lp, Xp = _setup(1000, 9400, 300)
    E = np.random.default_rng(4).standard_normal((300, 2))
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th)
    info = fit.krige_info()
    st0, qf0 = fit.krige_core(lp, Xp)
    fit.krige_joint_core(lp, Xp, iiderrors=E)           # the hand-off scratch of the factorisation exists before the baseline
    _free_bytes()
    base = _free_bytes()
    fit.krige_joint_core(lp, Xp, iiderrors=E)
    after = _free_bytes()
    assert abs(base - after) <= 64 * 2 ** 20, (base, after)
    assert fit.krige_info() == info
    st1, qf1 = fit.krige_core(lp, Xp)
    assert np.array_equal(st0, st1) and np.array_equal(qf0, qf1)
    fit.close()


def test_joint_failure_recovery_and_refusals():
    """The pinned request (krige_joint_reference.failing_request, n = 600, m = 4): with one draw the call returns -5, the
    message starts with the entry's name and names minor 2, the outputs are untouched; with nsim = 0 it returns a cov whose
    [0, 1] entry is below -1; with locs_unobs = None and one draw it then succeeds.  Refused: no state, a released state,
    a taper handle."""
    import cocons_amd as ca
    from cocons_amd import _lib
    from cocons_amd import workloads as wl
    from test_gpu_parity import _taper_pattern
    locs, X, th, z, _, _ = _setup(600, 8500, 4)
    lp, lu, Xp = ref.failing_request(locs)
    lpf, luf, Xpf = (np.asfortranarray(a) for a in (lp, lu, Xp))
    E = np.asfortranarray(np.random.default_rng(6).standard_normal((4, 1)))
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    with pytest.raises(_lib.CoconsHipError, match="cocons_krige_joint: no kriging state.*cocons_krige_prepare"):
        fit.krige_joint_core(lp, Xp)
    fit.krige_prepare(th)
    st, cov, sims = np.full(4, 7.0), np.full((4, 4), 7.0, order="F"), np.full((4, 1), 7.0, order="F")
    rc = fit._L.cocons_krige_joint(fit._h, 4, _p(lpf), _p(Xpf), _p(luf), _p(st), _p(cov), 1, _p(E), _p(sims))
    msg = _lib.last_error()
    assert rc == -5, (rc, msg)
    assert msg.startswith("cocons_krige_joint:") and "minor 2" in msg, msg
    assert np.all(st == 7.0) and np.all(cov == 7.0) and np.all(sims == 7.0)
    with pytest.raises(ca.KrigeJointNotPositiveDefinite, match="minor 2"):
        fit.krige_joint_core(lp, Xp, lu, E)
    st0, cov0, _ = fit.krige_joint_core(lp, Xp, lu)
    assert cov0[0, 1] < -1 and cov0[0, 0] > 0
    st1, cov1, sims1 = fit.krige_joint_core(lp, Xp, None, E)
    assert np.array_equal(st0, st1) and np.all(np.isfinite(sims1)) and np.all(np.linalg.eigvalsh(cov1) > 0)
    fit.krige_release()
    with pytest.raises(_lib.CoconsHipError, match="cocons_krige_joint: no kriging state"):
        fit.krige_joint_core(lp, Xp)
    fit.close()

    ci, rp, ent = _taper_pattern(locs, 0.25)
    tf = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, ent)
    st = np.full(4, 7.0)
    rc = tf._L.cocons_krige_joint(tf._h, 4, _p(lpf), _p(Xpf), None, _p(st), None, 0, None, None)
    assert rc == -1 and _lib.last_error().startswith("cocons_krige_joint: not available on a taper fit")
    assert np.all(st == 7.0)
    tf.close()


def test_glue_krige_joint_matches_krige_joint_core():
    """`_cocons_hip_krige_joint` through the R stub: the bits of krige_joint_core, with and without locs_unobs, draws and
    cov."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    from test_glue_exec import RStub
    R = RStub()
    locs, X, th, z, lp, Xp = _setup(300, 9600, 200)
    lu = lp + 0.01
    E = np.random.default_rng(7).standard_normal((200, 2))
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    fit.krige_prepare(th)
    want = fit.krige_joint_core(lp, Xp, lu, E)
    want_plain = fit.krige_joint_core(lp, Xp)
    fit.close()
    h = R.call("_cocons_hip_fit_create", R.real(locs), R.real(X), R.real(z[:, None]), R.nil, R.real(list(wl.SMOOTH_LIMITS)),
               R.integer([0]))
    st = R.value(R.call("_cocons_hip_krige_prepare", h, R.theta(th), R.real(th["mean"]), R.integer([1]), R.integer([0])))
    assert int(st[0][0]) == 0
    rc, st, cov, sims = R.value(R.call("_cocons_hip_krige_joint", h, R.real(lp), R.real(Xp), R.real(lu), R.real(E),
                                       R.integer([1])))
    assert int(rc[0]) == 0
    assert np.array_equal(st, want[0]) and np.array_equal(cov, want[1]) and np.array_equal(sims, want[2])
    rc, st, cov, sims = R.value(R.call("_cocons_hip_krige_joint", h, R.real(lp), R.real(Xp), R.nil, R.nil, R.integer([1])))
    assert int(rc[0]) == 0 and sims is None
    assert np.array_equal(st, want_plain[0]) and np.array_equal(cov, want_plain[1])
    rc, st, cov, sims = R.value(R.call("_cocons_hip_krige_joint", h, R.real(lp), R.real(Xp), R.real(lu), R.real(E),
                                       R.integer([0])))
    assert int(rc[0]) == 0 and cov is None and np.array_equal(sims, want[2])
    R.call("_cocons_hip_krige_release", h)
    with pytest.raises(RuntimeError, match="cocons_krige_joint"):
        R.call("_cocons_hip_krige_joint", h, R.real(lp), R.real(Xp), R.nil, R.nil, R.integer([1]))
    R.L.stub_gc(0, None)
