"""GPU parity tests at sizes where the ENGINE schedule runs (more than four 128-column tiles: the resident diagonal-block
engine, the dynamic tile order, the GEMM panel) -- every entry point against the CPU oracle, which still finishes in
seconds at n = 1024 ... 4096.  Closes the thin spots of the small-n tests (tests/test_gpu_parity.py run n = 260 ... 700,
where the plain schedule is used).  The autouse fixture in conftest.py asserts that no hand-off timed out."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENGINE_OFF = os.environ.get("COCONS_ENGINE", "1") == "0"      # (tools/gpu_switch_matrix.sh runs the suite that way too)

N2LL_RTOL = 1e-8


def _grid(gx, gy=None):
    from cocons_amd import workloads as wl
    locs = wl.grid_locs(gx, gy)
    sc = wl.design_from_locs(locs)
    return locs, sc


def test_c5_shifted_grid_n2048_vs_oracle(oracle):
    """cocoPredict dense (R/predict.R:136-183) in the shape of BASELINE config C5 -- a grid, predictions on the grid shifted
    by half a cell -- at n = m = 2048 against the CPU restatement: stochastic part and predictive variances."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, sc = _grid(64, 32)
    X = sc["std.covs"]
    th = wl.theta_full()
    th["mean"] = np.array([0.3, -0.1, 0.2])
    z = wl.synthetic_z(2048)
    lp = locs + np.array([0.5 / 63, 0.5 / 31])
    Xp = wl.design_from_locs(lp, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    got = ca.cocoPredict_dense(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z, fit=fit)
    assert fit.engine_state()["active"] or ENGINE_OFF
    want = oracle.cocoPredict_dense(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z)
    assert np.allclose(got["systematic"], want["systematic"], rtol=1e-13, atol=0)
    assert np.max(np.abs(got["stochastic"] - want["stochastic"])) < 1e-9 * np.max(np.abs(want["stochastic"]))
    vg, vw = got["sd.pred"] ** 2, want["sd.pred"] ** 2
    assert np.max(np.abs(vg - vw)) < 1e-11 * np.max(vw)


def test_profile_and_reml_n4096_q3_vs_oracle(oracle):
    """GetNeg2loglikelihoodProfile / ...REML (R/neg2loglikelihood.R:127-165, 241-291) on the 64 x 64 grid with q = 3
    trend columns and two realisations: the bordered factorisation with r + q rows under the matrix on the engine
    schedule, against the CPU restatement (chol2inv and the n x n P matrix there)."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n = 4096
    locs, sc = _grid(64)
    X = sc["std.covs"]
    th = wl.theta_full()
    rng = np.random.default_rng(4096)
    z = rng.standard_normal((n, 2)) + 0.5 + (X @ np.array([0.0, 0.4, -0.3]))[:, None]
    pp = wl.par_pos_full()
    tv = wl.theta_vector_from_lists(th, pp)
    lam = (0.1, 0.0, 0.3)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS, x_betas=X)
    got = ca.GetNeg2loglikelihoodProfile(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=fit)
    assert fit.engine_state()["active"] or ENGINE_OFF
    want = oracle.GetNeg2loglikelihoodProfile(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam)
    assert abs(got - want) <= N2LL_RTOL * abs(want)
    got = ca.GetNeg2loglikelihoodREML(tv, pp, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)
    want = oracle.GetNeg2loglikelihoodREML(tv, pp, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam)
    assert abs(got - want) <= N2LL_RTOL * abs(want)


def test_cocoSim_conditional_n2048_m512_vs_oracle(oracle):
    """cocoSim, conditional branch (R/sim.R:84-127), n = 2048 observed and m = 512 new locations: ONE joint Cholesky of order
    2560 on the engine schedule against solve + Schur complement + chol + cocoPredict(type = 'mean') on the CPU."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    n, m = 2048, 512
    rng = np.random.default_rng(2048)
    locs = rng.uniform(0, 1, size=(n, 2))
    sc = wl.design_from_locs(locs)
    X = sc["std.covs"]
    th = wl.theta_full(scale0=np.log(0.1))
    th["mean"] = np.array([0.3, -0.2, 0.1])
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = wl.design_from_locs(lp, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    newdataset = np.column_stack([lp, rng.standard_normal((m, 2))])
    z = rng.standard_normal(n)
    E = rng.standard_normal((m, 4))
    got = ca.cocoSim_cond_dense(th, locs, lp, newdataset, X, Xp, wl.SMOOTH_LIMITS, z, E)
    want = oracle.cocoSim_cond_dense(th, locs, lp, newdataset, X, Xp, wl.SMOOTH_LIMITS, z, E)
    assert got.shape == (m, 4)
    assert np.max(np.abs(got - want)) < 1e-8 * np.max(np.abs(want))


def test_fuzz_random_parameters_n1024_r3(oracle):
    """12 random parameter sets (ranges 0.03 ... 0.6, nuggets 1e-4 ... 0.1, three pairs of smoothness limits, strong
    covariate effects) at n = 1024 with r = 3 realisations: the engine schedule within the north-star tolerance of the
    CPU path, or both sides agree that the Cholesky fails."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    rng = np.random.default_rng(1024)
    n = 1024
    locs = rng.uniform(0, 1, size=(n, 2))
    X = wl.design_from_locs(locs)["std.covs"]
    z = rng.standard_normal((n, 3))
    pp = wl.par_pos_full()
    worst, nfail, used_engine = 0.0, 0, 0
    for it in range(12):
        lim = [(0.5, 2.5), (0.3, 1.2), (1.0, 3.0)][it % 3]
        th = wl.theta_full(scale0=np.log(rng.uniform(0.03, 0.6)))
        for k in ("std.dev", "scale", "aniso", "tilt", "smooth"):
            th[k] = th[k] + np.r_[0.0, rng.normal(0, 0.4, size=2)]
        th["nugget"] = np.array([np.log(10 ** rng.uniform(-4, -1)), 0.0, 0.0])
        tv = wl.theta_vector_from_lists(th, pp)
        fit = ca.CoconsFit(locs, X, z, lim)
        got = ca.GetNeg2loglikelihood(tv, pp, locs, X, lim, z, n, (0.1, 0.1, 0.1), fit=fit)
        used_engine += int(fit.engine_state()["active"])
        want = oracle.GetNeg2loglikelihood(tv, pp, locs, X, lim, z, n, (0.1, 0.1, 0.1))
        if want == 1e6 or got == 1e6:
            assert got == want, (it, got, want)
            nfail += 1
            continue
        worst = max(worst, abs(got - want) / abs(want))
    assert worst <= N2LL_RTOL, worst
    assert nfail < 5 and (used_engine == 12 or ENGINE_OFF)


def test_taper_objective_n10000_vs_host_sparse_lu(oracle):
    """GetNeg2loglikelihoodTaper (R/neg2loglikelihood.R:20-53) at n = 10 000 (the 100 x 100 grid, Wendland-1 taper of range
    0.06, ~1 % dense): the band-limited factorisation on the device against a sparse LU (SuperLU) of the SAME tapered matrix
    on the host, whose entries come from the CPU restatement of cov_rns_taper."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    g, delta = 100, 0.06
    n = g * g
    locs, sc = _grid(g)
    X = sc["std.covs"]
    th = wl.theta_full()
    z = wl.synthetic_z(n)
    ci, rp, ent = [], [1], []
    cell = {}
    for i, (x, y) in enumerate(locs):
        cell.setdefault((int(x / delta), int(y / delta)), []).append(i)
    for i, (x, y) in enumerate(locs):
        cx, cy = int(x / delta), int(y / delta)
        cand = np.array(sorted(j for a in (-1, 0, 1) for b in (-1, 0, 1) for j in cell.get((cx + a, cy + b), [])))
        d = np.sqrt(np.sum((locs[cand] - locs[i]) ** 2, axis=1))
        keep = d <= delta
        h = d[keep] / delta
        ci.extend((cand[keep] + 1).tolist())
        ent.extend(((1 - h) ** 4 * (4 * h + 1)).tolist())
        rp.append(len(ci) + 1)
    ci, rp, ent = np.array(ci, dtype=np.int32), np.array(rp, dtype=np.int32), np.array(ent)
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, ent)
    got, parts = fit.neg2loglik_core(th)
    vals = ent * oracle.cov_rns_taper(th, locs, X, ci, rp, wl.SMOOTH_LIMITS)
    S = sp.csr_matrix((vals, ci - 1, rp - 1), shape=(n, n)).tocsc()
    lu = spl.splu(S, permc_spec="MMD_AT_PLUS_A", options=dict(SymmetricMode=True))
    resid = z - X @ th["mean"]
    quad = float(resid @ lu.solve(resid))
    logdet = float(np.sum(np.log(np.abs(lu.U.diagonal()))))
    want = n * np.log(2 * np.pi) + logdet + quad
    assert abs(got - want) <= N2LL_RTOL * abs(want)
    assert abs(2 * parts[0] - logdet) <= 1e-9 * abs(logdet) and abs(parts[1] - quad) <= 1e-8 * abs(quad)


@pytest.mark.shared_gpu          # (exempt from the autouse "no time-out" check: this test provokes one on purpose)
def test_engine_timeout_is_survived_counted_and_backed_off():
    """A genuine hand-off time-out (the gate kernel is made to wait for a word nobody raises: 5 ms, abort code 0x600) must
    cost ONE evaluation its engine schedule and nothing else: the value is the plain schedule's, the time-out is counted and
    its code kept (cocons_fit_engine_state), two operations -- the repeat of this one and the next -- take the plain schedule
    (back-off, doubling with consecutive time-outs), then the engine is used again.  Round 2's fall-back was silent and
    permanent."""
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    if ENGINE_OFF:
        pytest.skip("COCONS_ENGINE=0")
    L = _lib.load()
    locs, sc = _grid(48)                         # n = 2304: 18 tiles, engine schedule
    X = sc["std.covs"]
    z = wl.synthetic_z(locs.shape[0])
    th = wl.theta_full()
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        v0 = fit.neg2loglik_core(th)[0]
        st = fit.engine_state()
        assert st == {"active": True, "retries": 0, "last_abort": 0}
        _lib.check(L.cocons_debug_tune(b"gate_sabotage", 1), "tune")
        v1 = fit.neg2loglik_core(th)[0]
        st = fit.engine_state()
        assert st["retries"] == 1 and st["last_abort"] == 0x600 and not st["active"], st
        assert abs(v1 - v0) <= 1e-12 * abs(v0)
        # back-off after the first time-out: 2 operations on the plain schedule, the repeat inside the call above being one
        assert abs(fit.neg2loglik_core(th)[0] - v0) <= 1e-12 * abs(v0)
        assert not fit.engine_state()["active"]
        v4 = fit.neg2loglik_core(th)[0]
        st = fit.engine_state()
        assert st["active"] and st["retries"] == 1, st
        assert abs(v4 - v0) <= 1e-12 * abs(v0)
    finally:
        L.cocons_debug_tune(b"gate_sabotage", 0)
        fit.close()


@pytest.mark.shared_gpu          # (exempt from the autouse "no time-out" check: the second half provokes one on purpose)
def test_late_host_is_waited_for_and_a_short_bound_records_0x112(oracle):
    """The time-out round 5's first GPU run recorded (`test_profile_and_reml_n4096_q3_vs_oracle: retries=1 last_abort=0x112`:
    the engine gave up waiting for tile 18's input word) was put down to a host thread throttled in the middle of enqueueing
    an evaluation -- the launches that raise in[18] came later than the 100 ms the engine then waited.  Here the cause is
    produced on purpose, in the same configuration (Profile at n = 4096, q = 3, two realisations): the enqueueing thread sleeps
    250 ms in front of the launches that raise in[18] (cocons_debug_tune "host_delay_us" / "host_delay_tile").
    (a) Under the shipped bound of the host-paced waits (3 s) the evaluation finishes ON THE ENGINE SCHEDULE, no time-out, the
    value equal to the oracle's.  (b) With the bound put back to 100 ms the engine gives up with exactly 0x112 -- or its partner,
    which waits for the same late launches one word further, with 0x212 --, the operation is repeated on the plain schedule
    (counted), and the value is still right."""
    import time
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    if ENGINE_OFF:
        pytest.skip("COCONS_ENGINE=0")
    L = _lib.load()
    n = 4096
    locs, sc = _grid(64)
    X = sc["std.covs"]
    th = wl.theta_full()
    rng = np.random.default_rng(4096)
    z = rng.standard_normal((n, 2)) + 0.5 + (X @ np.array([0.0, 0.4, -0.3]))[:, None]
    pp = wl.par_pos_full()
    tv = wl.theta_vector_from_lists(th, pp)
    lam = (0.1, 0.0, 0.3)
    want = oracle.GetNeg2loglikelihoodProfile(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS, x_betas=X)
    try:
        v0 = ca.GetNeg2loglikelihoodProfile(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=fit)
        assert fit.engine_state() == {"active": True, "retries": 0, "last_abort": 0}
        assert abs(v0 - want) <= N2LL_RTOL * abs(want)
        _lib.check(L.cocons_debug_tune(b"host_delay_tile", 18), "tune")
        _lib.check(L.cocons_debug_tune(b"host_delay_us", 250000), "tune")
        t0 = time.perf_counter()
        v1 = ca.GetNeg2loglikelihoodProfile(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=fit)
        dt = time.perf_counter() - t0
        if dt < 0.25:            # (COCONS_DAG_MIN_TILES=0: every step under the persistent launch -- the classic loop the hook lives in is not reached)
            pytest.skip("no step of this factorisation runs the classic loop under the switches in force")
        st = fit.engine_state()
        assert st == {"active": True, "retries": 0, "last_abort": 0}, st
        assert v1 == v0                                         # the same schedule, the same bits
        # (b) the bound of rounds 2-4
        _lib.check(L.cocons_debug_tune(b"engine_in_wait_ms", 100), "tune")
        v2 = ca.GetNeg2loglikelihoodProfile(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=fit)
        st = fit.engine_state()
        # (the engine waits for in[18], its partner for in[19] -- both raised by the late launches: whichever of the two runs out
        # first leaves its code, 0x112 or 0x212)
        # (with three-launch panels -- COCONS_PANEL_FUSED=0, or COCONS_ENGINE_PAIR=0 -- the next diagonal block is updated by the
        # update launch instead of inside the panel's, and the late launches are the ones that raise in[16] / in[17]: 0x110 / 0x210)
        code = st["last_abort"]
        assert st["retries"] == 1 and (code & 0xf00) in (0x100, 0x200) and (code & 0xff) in (16, 17, 18, 19) and not st["active"], st
        if not any(os.environ.get(k) for k in ("COCONS_PANEL_FUSED", "COCONS_ENGINE_PAIR")):
            assert code in (0x112, 0x212), hex(code)
        assert abs(v2 - want) <= N2LL_RTOL * abs(want)
    finally:
        L.cocons_debug_tune(b"host_delay_us", 0)
        L.cocons_debug_tune(b"host_delay_tile", -1)
        L.cocons_debug_tune(b"engine_in_wait_ms", 0)
        fit.close()


@pytest.mark.shared_gpu          # (seven live handles = fourteen streams on four hardware queues: a hand-off may time out and be repeated)
def test_handles_created_used_and_destroyed_from_three_threads(record_property):
    """The threading contract of the boundary (include/cocons_hip.h): different handles may be created, used and destroyed from
    different threads at the same time.  A new handle's stream self-test launches probe kernels on the streams of OTHER live
    handles (api_handle.hip engine_warm) -- until round 5 without holding anything, so that a handle could be used or destroyed under
    the probe (the advisor's finding); now it takes the other handle's operation lock, and a busy handle is skipped.  Three
    threads churn through handles of engine-schedule size while each also evaluates on its own: every value must equal the
    single-threaded one and nothing may crash or hang.  (Hand-off time-outs are recorded, not forbidden: with this many live
    handles streams share hardware queues, and an engine that shares one with another handle's main stream is ended by its bounded
    waits and repeated on the plain schedule -- DESIGN.md section 4a.)"""
    import threading
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, sc = _grid(32)                         # n = 1024: 8 tiles, engine schedule
    X = sc["std.covs"]
    z = wl.synthetic_z(locs.shape[0])
    th = wl.theta_full()
    ref_fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    ref = ref_fit.neg2loglik_core(th)[0]
    errors, retries = [], []

    def churn(seed):
        try:
            keep = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
            for it in range(8):
                f = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)       # (its creation probes the other threads' handles)
                for g in (f, keep):
                    v = g.neg2loglik_core(th)[0]
                    if abs(v - ref) > 1e-12 * abs(ref):
                        errors.append((seed, it, v))
                retries.append(f.engine_state()["retries"])
                f.close()
            retries.append(keep.engine_state()["retries"])
            keep.close()
        except Exception as e:                   # noqa: BLE001
            errors.append((seed, repr(e)))

    ts = [threading.Thread(target=churn, args=(i,)) for i in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "a thread hangs"
    assert not errors, errors
    record_property("engine_timeouts", sum(retries))
    assert abs(ref_fit.neg2loglik_core(th)[0] - ref) <= 1e-12 * abs(ref)
    ref_fit.close()


def test_front_padding_n2115_all_entry_points_vs_oracle(oracle):
    """n = 45 x 47 = 2115 is not a multiple of 128: the handle keeps 61 placeholder observations IN FRONT of the caller's
    (unit columns, api_handle.hip fit_create_impl) instead of identity padding behind them.  Every entry point that runs on that
    layout, on the engine schedule, against the CPU restatement: -2 loglik (two realisations), Profile and REML with q = 3,
    the kriging core, and the status of a failing factorisation (reported in the caller's numbering)."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, sc = _grid(45, 47)
    n = locs.shape[0]
    assert n == 2115 and n % 128 != 0
    X = sc["std.covs"]
    th = wl.theta_full()
    th["mean"] = np.array([0.2, -0.1, 0.05])
    rng = np.random.default_rng(2115)
    z = rng.standard_normal((n, 2)) + (X @ np.array([0.1, 0.4, -0.3]))[:, None]
    pp = wl.par_pos_full()
    pp["mean"] = [True] * 3
    tv = np.concatenate([th["mean"], wl.theta_vector_from_lists(th, wl.par_pos_full())])
    lam = (0.1, 0.0, 0.3)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS, x_betas=X)
    got = ca.GetNeg2loglikelihood(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)
    assert fit.engine_state()["active"] or ENGINE_OFF
    want = oracle.GetNeg2loglikelihood(tv, pp, locs, X, wl.SMOOTH_LIMITS, z, n, lam)
    assert abs(got - want) <= 1e-11 * abs(want)
    pq = wl.par_pos_full()
    tq = wl.theta_vector_from_lists(th, pq)
    got = ca.GetNeg2loglikelihoodProfile(tq, pq, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=fit)
    want = oracle.GetNeg2loglikelihoodProfile(tq, pq, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam)
    assert abs(got - want) <= N2LL_RTOL * abs(want)
    got = ca.GetNeg2loglikelihoodREML(tq, pq, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)
    want = oracle.GetNeg2loglikelihoodREML(tq, pq, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam)
    assert abs(got - want) <= N2LL_RTOL * abs(want)
    lp = locs[:300] + np.array([0.4 / 44, 0.4 / 46])
    Xp = wl.design_from_locs(lp, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    fit1 = ca.CoconsFit(locs, X, z[:, 0], wl.SMOOTH_LIMITS)
    got = ca.cocoPredict_dense(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z[:, 0], fit=fit1)
    want = oracle.cocoPredict_dense(th, locs, lp, X, Xp, wl.SMOOTH_LIMITS, z[:, 0])
    assert np.max(np.abs(got["stochastic"] - want["stochastic"])) < 1e-9 * np.max(np.abs(want["stochastic"]))
    vg, vw = got["sd.pred"] ** 2, want["sd.pred"] ** 2
    assert np.max(np.abs(vg - vw)) < 1e-11 * np.max(vw)
    # a matrix that is not positive definite: two coincident locations without a nugget -- the failing minor is
    # reported between 1 and n (the placeholder columns in front are not counted)
    locs2 = locs.copy()
    locs2[1500] = locs2[1499]
    X2 = X.copy()
    X2[1500] = X2[1499]
    th2 = {k: np.array(v, dtype=float) for k, v in th.items()}
    th2["nugget"] = np.array([-np.inf, 0.0, 0.0])
    fit2 = ca.CoconsFit(locs2, X2, z[:, 0], wl.SMOOTH_LIMITS)
    try:
        v = fit2.neg2loglik_core(th2)[0]   # exactly singular: whether the pivot at the duplicate comes out <= 0 or a rounding
    except ca.CholeskyError as e:          # error above it depends on the schedule (LAPACK's dpotrf is no different); the default
        assert 1 <= e.minor <= n           # schedule reports it, and then in the caller's numbering
    else:
        assert np.isfinite(v)              # a rounding error above zero: a finite value, as dpotrf would return
    fit2.close()
    # ... and a matrix whose failure is NOT a matter of rounding: fixed smoothness 1 (not one of the closed forms) leaves every
    # off-diagonal entry equal to the diagonal (SURVEY 8a#6 quirk i), so with constant variance the second pivot is exactly
    # 1 - 1 * 1 = 0: a report is mandatory and names minor 2
    th3 = {k: np.zeros(3) for k in th}
    th3["scale"] = np.array([np.log(0.05), 0.0, 0.0])
    th3["nugget"] = np.array([-np.inf, 0.0, 0.0])
    th3["mean"] = np.zeros(3)
    fit3 = ca.CoconsFit(locs, X, z[:, 0], (1.0, 1.0))
    with pytest.raises(ca.CholeskyError) as ei:
        fit3.neg2loglik_core(th3)
    assert ei.value.minor == 2
    fit3.close()


def test_repeated_evaluations_are_bit_identical():
    """No floating-point atomics and no schedule-dependent order of summation: the same parameters give the same bits, on
    the engine schedule (dynamic tile order included), also after another entry point used -- and dirtied -- the rows under
    the matrix of the same handle."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, sc = _grid(50, 47)                     # n = 2350: front padding and slots in use
    X = sc["std.covs"]
    z = wl.synthetic_z(locs.shape[0])
    th = wl.theta_full()
    th2 = {k: np.array(v, dtype=float) for k, v in th.items()}
    th2["scale"][0] += 0.07
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    a0, b0 = fit.neg2loglik_core(th)[0], fit.neg2loglik_core(th2)[0]
    lp = locs[:100] + 0.3 / 49
    Xp = wl.design_from_locs(lp, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    p0 = fit.predict_core(th, lp, Xp)[0].copy()
    for _ in range(3):
        assert fit.neg2loglik_core(th)[0] == a0
        assert fit.neg2loglik_core(th2)[0] == b0
        assert np.array_equal(fit.predict_core(th, lp, Xp)[0], p0)
    assert a0 != b0


@pytest.mark.parametrize("gx,gy", [(28, 25), (45, 47), (64, 64), (72, 64)])
def test_engine_pair_same_bits_as_one_workgroup(gx, gy):
    """The engine as a PAIR of workgroups (COCONS_ENGINE_PAIR, round 5: the second one follows the first tile's factorisation
    column block by column block and factors the second tile, chol.hip engine_partner_loop) performs the same operations on
    the same operands in the same order as the one-workgroup engine: -2 loglik and the reduction outputs are BIT-identical; sizes with a last block of one tile, right-hand sides in slots and under the
    matrix, two realisations."""
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    if ENGINE_OFF:
        pytest.skip("COCONS_ENGINE=0")
    L = _lib.load()
    locs, sc = _grid(gx, gy)
    n = locs.shape[0]
    X = sc["std.covs"]
    th = wl.theta_full()
    th["mean"] = np.array([0.1, -0.2, 0.05])
    rng = np.random.default_rng(n + 1)
    z = rng.standard_normal((n, 2)) + (X @ np.array([0.2, 0.3, -0.1]))[:, None]
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        _lib.check(L.cocons_debug_tune(b"engine_pair", 1), "tune")
        v1, p1 = fit.neg2loglik_core(th)
        v1b = fit.neg2loglik_core(th)[0]
        assert fit.engine_state()["active"]
        _lib.check(L.cocons_debug_tune(b"engine_pair", 0), "tune")
        v0, p0 = fit.neg2loglik_core(th)
        assert fit.engine_state()["active"]
        assert v1 == v0 and v1b == v1 and np.array_equal(p1, p0)
    finally:
        _lib.check(L.cocons_debug_tune(b"engine_pair", int(os.environ.get("COCONS_ENGINE_PAIR", "1"))), "tune")


@pytest.mark.parametrize("gx,gy", [(33, 31), (45, 47), (64, 64), (72, 64)])
def test_following_panel_same_bits_as_three_launches(gx, gy):
    """The panel of a two-tile block in one launch whose strips follow the engine pair's tiles (COCONS_PANEL_FUSED, chol.hip
    panel_pair_kernel: solve | in-panel update | solve with both strips in registers), with two workgroups per strip in every
    panel and with one, against the three launches it replaces: same operations, same order -- identical bits."""
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    if ENGINE_OFF:
        pytest.skip("COCONS_ENGINE=0")
    L = _lib.load()
    locs, sc = _grid(gx, gy)
    n = locs.shape[0]
    X = sc["std.covs"]
    th = wl.theta_full()
    th["mean"] = np.array([0.1, -0.2, 0.05])
    rng = np.random.default_rng(n + 2)
    z = rng.standard_normal((n, 2)) + (X @ np.array([0.2, 0.3, -0.1]))[:, None]
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        _lib.check(L.cocons_debug_tune(b"panel_fused", 1), "tune")
        _lib.check(L.cocons_debug_tune(b"panel_split", 1), "tune")       # (two workgroups per strip in EVERY panel: the default asks for 32 strips)
        v1, p1 = fit.neg2loglik_core(th)
        assert fit.engine_state()["active"]
        _lib.check(L.cocons_debug_tune(b"panel_split", 0), "tune")       # (one workgroup per strip instead of two)
        v4, p4 = fit.neg2loglik_core(th)
        assert v4 == v1 and np.array_equal(p4, p1)
        _lib.check(L.cocons_debug_tune(b"panel_fused", 0), "tune")
        v0, p0 = fit.neg2loglik_core(th)
        assert fit.engine_state()["active"]
        assert v1 == v0 and np.array_equal(p1, p0)
    finally:
        _lib.check(L.cocons_debug_tune(b"panel_fused", int(os.environ.get("COCONS_PANEL_FUSED", "1"))), "tune")
        _lib.check(L.cocons_debug_tune(b"panel_split", int(os.environ.get("COCONS_PANEL_SPLIT", "32"))), "tune")


@pytest.mark.parametrize("gx,gy,engine", [(20, 20, 1), (33, 31, 0), (45, 47, 0), (64, 64, 0)])
def test_potrf_follow_same_bits_as_two_launches(gx, gy, engine):
    """Tile factorisation and the panel solve below it in one launch whose solve workgroups follow the factorisation through the
    tile's mailbox (COCONS_POTRF_FOLLOW, chol.hip potrf_follow_kernel) against the two launches: identical bits -- on the plain
    schedule (engine off: every tile; an odd number of 64-row strips, right-hand sides in slots and under the matrix) and on a
    small problem that never uses the engine."""
    import cocons_amd as ca
    from cocons_amd import _lib, workloads as wl
    L = _lib.load()
    locs, sc = _grid(gx, gy)
    n = locs.shape[0]
    X = sc["std.covs"]
    th = wl.theta_full()
    th["mean"] = np.array([0.1, -0.2, 0.05])
    rng = np.random.default_rng(n + 3)
    z = rng.standard_normal((n, 2)) + (X @ np.array([0.2, 0.3, -0.1]))[:, None]
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        _lib.check(L.cocons_debug_tune(b"engine", engine), "tune")
        _lib.check(L.cocons_debug_tune(b"potrf_follow", 1), "tune")
        v1, p1 = fit.neg2loglik_core(th)
        v1b = fit.neg2loglik_core(th)[0]
        _lib.check(L.cocons_debug_tune(b"potrf_follow", 0), "tune")
        v0, p0 = fit.neg2loglik_core(th)
        assert v1 == v0 and v1b == v1 and np.array_equal(p1, p0)
        assert fit.engine_state()["retries"] == 0
    finally:
        _lib.check(L.cocons_debug_tune(b"engine", int(os.environ.get("COCONS_ENGINE", "1"))), "tune")
        _lib.check(L.cocons_debug_tune(b"potrf_follow", int(os.environ.get("COCONS_POTRF_FOLLOW", "1"))), "tune")
