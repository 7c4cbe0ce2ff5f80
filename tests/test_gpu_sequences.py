"""Every entry of a fit handle behind every other one, on ONE handle, held to fresh-handle bits; and the caller's stream.

tests/sequence_cases.py defines the kinds of events, the circuit in which every ordered pair of kinds is adjacent exactly once,
and the model of the held kriging state.  Here each circuit runs on one handle (in consecutive parts where it would take too
long: a part starts on a fresh handle with the last event of the part before, so no pair is lost).  After EVERY event every output
array -- status codes and failing minors included; for a failure the exception's type and minor -- is compared bit for bit with
the referee: the same event on a fresh handle, or for an apply / joint event a fresh handle plus the one prepare the model
names.  Referees are built once per (kind, model state), the fresh handle closed at once.  krige_info()["prepared"] is held
against the model after every event, engine_state()["retries"] == 0 at the end.

Kinds compared by a tolerance: none (TOLERANCE is empty).  An entry whose bits are found to depend on history gets its cause
written beside its kind in tests/sequence_cases.py and, only for a legitimate difference of summation order, an entry here
that names the constant of its own existing test.

The caller's stream (cocons_fit_set_stream, cocons_fit_stream, cocons_fit_sync): two "install a caller's stream" kinds join the
circuits of the plain-schedule handles (n = 130 dense, n = 640 taper); the direct checks and the engine-size test are at the
end of the file.  Streams come from torch.cuda.Stream().

Where the torch work runs.  torch ships a HIP runtime of its own, and a process can hold only one: whichever of torch and
libcocons_hip.so is loaded FIRST brings the runtime both then use (bench.py imports torch first).  In a pytest session other
tests have loaded the library long before, and torch would then find no device.  So everything that needs torch -- the two
circuits with stream kinds, the direct checks, the engine-size test -- runs as jobs of ONE child process that imports torch
first (this file run as a script, started once per session by the fixture torch_jobs); the tests below assert what their job
reported.  The child holds the same rules: every handle closes with retries == 0.

Every test prints one line that starts with `sequences-report` (tests/golden/SEQUENCES_REPORT.md is made from them)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sequence_cases as SC  # noqa: E402
import taper_envelope_cases as TE  # noqa: E402

pytestmark = pytest.mark.gpu

# problem -> (handle kind, stream kinds in the circuit, consecutive parts)
PROBLEMS = {
    "dense130": ("dense", True, 1),
    "dense256": ("dense", False, 1),
    "dense700": ("dense", False, 1),
    "taper_n129": ("taper", False, 1),
    "taper_n640": ("taper", True, 1),
    "taper_irregular": ("taper", False, 1),
}
RUNS = [(key, part) for key, (_, streams, parts) in PROBLEMS.items() if not streams for part in range(parts)]
STREAM_RUNS = [(key, part) for key, (_, streams, parts) in PROBLEMS.items() if streams for part in range(parts)]
TOLERANCE = {}                # kind -> (relative bound, the existing test it is imported from): empty, every kind is bitwise
SWITCHES = ("COCONS_SPATIAL_SORT", "COCONS_TAPER_RCM", "COCONS_TAPER_PACKED", "COCONS_TAPER_BAND", "COCONS_KRIGE_JOINT_DEPTH",
            "COCONS_ENGINE")

_REFEREES = {}                # (problem, kind, prepare) -> outcome
_STREAMS = []                 # the callers' streams of this module: made once, never destroyed before a handle that uses them


def _streams(count):
    import torch
    while len(_STREAMS) < count:
        _STREAMS.append(torch.cuda.Stream())
    return _STREAMS[:count]


# --------------------------------------------------------------------------- handles and calls
def _problem(key):
    return SC.dense_problem(int(key[5:])) if key.startswith("dense") else SC.taper_problem(key[6:])


def _fresh(monkeypatch, key):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    prob = _problem(key)
    if key.startswith("dense"):
        return ca.CoconsFit(prob.locs, prob.X, prob.z, wl.SMOOTH_LIMITS, x_betas=prob.X)
    if not prob.rcm:
        monkeypatch.setenv("COCONS_TAPER_RCM", "0")
    return ca.CoconsTaperFit(prob.locs, prob.X, prob.z, TE.SMOOTH_LIMITS, *prob.ref_taper)


def _close(fit):
    """close a handle; no engine hand-off may have timed out on it (what the suite's conftest asserts for every handle of a test,
    said here as well for the handles of the child process)"""
    try:
        state = fit.engine_state()
    finally:
        fit.close()
    assert state["retries"] == 0, state


def _calls(key):
    """kind -> the call on a handle (the arguments are sequence_cases's, fixed)"""
    prob = _problem(key)
    T = SC.thetas(prob.theta)
    r = prob.z.shape[1]
    if key.startswith("dense"):
        A = SC.dense_args(prob.n)
        kz = {k.name: SC.z_col_of(k, r) for k in SC.DENSE_KINDS}
        return {
            "value_a": lambda f: f.neg2loglik_core(T["a"]),
            "value_b": lambda f: f.neg2loglik_core(T["b"]),
            "grad_a": lambda f: f.neg2loglik_grad_core(T["a"]),
            "profile_a": lambda f: f.neg2loglik_profile_core(T["a"]),
            "reml_b": lambda f: f.neg2loglik_reml_core(T["b"], 3),
            "profile_grad_b": lambda f: f.neg2loglik_profile_grad_core(T["b"]),
            "reml_grad_a": lambda f: f.neg2loglik_reml_grad_core(T["a"], 3),
            "fisher3_a": lambda f: f.fisher_core(T["a"], A["dirs"]),
            "fisher_reml_b": lambda f: f.fisher_reml_core(T["b"], A["dirs"]),
            "cv_loo_a": lambda f: f.cv_core(T["a"]),
            "cv_folds_b": lambda f: f.cv_core(T["b"], A["folds"]),
            "batch3": lambda f: f.neg2loglik_batch_core([T["a"], T["rank1"], T["b"]]),
            "predict70_a": lambda f: f.predict_core(T["a"], prob.lp, prob.Xp, z_col=kz["predict70_a"]),
            "predict300_b": lambda f: f.predict_core(T["b"], A["lp300"], A["Xp300"], z_col=kz["predict300_b"]),
            "prepare_a": lambda f: f.krige_prepare(T["a"], z_col=kz["prepare_a"], max_rows=64),
            "prepare_b_z1": lambda f: f.krige_prepare(T["b"], z_col=kz["prepare_b_z1"]),
            "prepare_npd": lambda f: f.krige_prepare(T["npd"], z_col=kz["prepare_npd"]),
            "krige70": lambda f: f.krige_core(prob.lp, prob.Xp),
            "joint70": lambda f: f.krige_joint_core(prob.lp, prob.Xp, iiderrors=A["E_joint"]),
            "release": lambda f: f.krige_release(),
            "cov_rows_a": lambda f: f.cov_rows(T["a"], A["rows"], cor=True),
            "sim_b": lambda f: f.sim_core(T["b"], A["E_sim"]),
            "sim_cond_a": lambda f: f.sim_cond_core(T["a"], prob.lp, prob.Xp, prob.lp, A["E_cond"]),
            "value_nan": lambda f: f.neg2loglik_core(T["nan"]),
            "value_npd": lambda f: f.neg2loglik_core(T["npd"]),
        }
    A = SC.taper_args(key[6:])
    kz = {k.name: SC.z_col_of(k, r) for k in SC.TAPER_KINDS}
    rows = A["rows"]
    return {
        "value_a": lambda f: f.neg2loglik_core(T["a"]),
        "value_b": lambda f: f.neg2loglik_core(T["b"]),
        "grad_a": lambda f: f.neg2loglik_grad_core(T["a"]),
        "fisher_exact_a": lambda f: f.fisher_core(T["a"], A["dirs"]),
        "fisher_probe8_b": lambda f: f.fisher_core(T["b"], A["dirs"], probes=A["probes"]),
        "cv_a": lambda f: f.cv_core(T["a"]),
        "predict_a": lambda f: f.predict_core(T["a"], prob.lp, prob.Xp, prob.pred_taper, z_col=kz["predict_a"]),
        "prepare_a": lambda f: f.krige_taper_prepare(T["a"], z_col=kz["prepare_a"], max_rows=64),
        "prepare_b_z1": lambda f: f.krige_taper_prepare(T["b"], z_col=kz["prepare_b_z1"]),
        "prepare_npd": lambda f: f.krige_taper_prepare(T["npd"], z_col=kz["prepare_npd"]),
        "krige": lambda f: f.krige_taper_core(prob.lp, prob.Xp, prob.pred_taper),
        "joint": lambda f: f.krige_taper_joint_core(prob.lp[rows], prob.Xp[rows], A["pred_rows"], A["uu_rows"],
                                                    iiderrors=A["E_joint"]),
        "release": lambda f: f.krige_taper_release(),
        "batch3": lambda f: f.neg2loglik_batch_core([T["a"], T["npd"], T["b"]]),
        "value_nan": lambda f: f.neg2loglik_core(T["nan"]),
        "value_npd": lambda f: f.neg2loglik_core(T["npd"]),
        "sim_own_b": lambda f: f.sim_core(T["b"], A["E_sim"]),
        "sim_pivot_a": lambda f: f.sim_core(T["a"], A["E_sim"], pivot=A["pivot"]),
    }


def _flat(out):
    if out is None:
        return []
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in (_flat(o) if o is not None else [None])]
    return [np.ascontiguousarray(out)]


def _outcome(call, fit):
    """("ok", the output arrays) or (the exception's type, its minor)"""
    import cocons_amd as ca
    from cocons_amd import _lib
    try:
        return ("ok", _flat(call(fit)))
    except ca.CholeskyError as e:
        return ("CholeskyError", e.minor)
    except _lib.CoconsHipError as e:
        return (type(e).__name__, None)


def _event(fit, key, name, calls):
    if name.startswith("stream_"):
        s = _streams(2)[int(name[-1])]
        fit.set_stream(s.cuda_stream)
        return ("ok", [np.array([fit.stream() == s.cuda_stream])])
    return _outcome(calls[name], fit)


def _referee(monkeypatch, key, ref, calls, kinds):
    """the outcome of the event on a fresh handle on its own stream (behind the one prepare the model names), built once"""
    if ref.kind.startswith("stream_"):
        return ("ok", [np.array([True])])
    at = (key, ref.kind, ref.prepare)
    if at not in _REFEREES:
        fit = _fresh(monkeypatch, key)
        try:
            if ref.prepare is not None:
                assert _outcome(calls[ref.prepare], fit) == ("ok", []), "the referee's prepare failed: " + ref.prepare
            out = _outcome(calls[ref.kind], fit)
        finally:
            _close(fit)
        # what the model (not the library) says about this outcome
        role = kinds[ref.kind].role
        if role == "apply":
            assert (out[0] == "ok") == (ref.prepare is not None), (ref, out[0])       # refused exactly without a state
            assert out[0] in ("ok", "CoconsHipError"), (ref, out[0])
        elif role == "prepare":
            assert out == ("ok", []), (ref, out[0])
        elif role == "prepare_fails":
            assert out[0] == "CholeskyError" and out[1] >= 1, (ref, out)
        elif ref.kind in ("value_nan", "value_npd"):
            assert out[0] == "CholeskyError", (ref, out)
        elif ref.kind == "batch3":
            st = out[1][1]
            assert out[0] == "ok" and st[0] == 0 and st[1] > 0 and st[2] == 0, (ref, st)     # the middle point alone fails
        else:
            assert out[0] == "ok", (ref, out)
        _REFEREES[at] = out
    return _REFEREES[at]


def _bits(a):
    return a.tobytes() if a is not None else None


def _difference(got, want):
    """None when the two outcomes are the same to the bit, else a text with the largest difference"""
    if got[0] != want[0]:
        return "outcome %r, the fresh handle's %r" % (got[:1] + ((got[1],) if got[0] != "ok" else ()),
                                                       want[:1] + ((want[1],) if want[0] != "ok" else ()))
    if got[0] != "ok":
        return None if got[1] == want[1] else "failing minor %r, the fresh handle's %r" % (got[1], want[1])
    if len(got[1]) != len(want[1]):
        return "%d outputs, the fresh handle's %d" % (len(got[1]), len(want[1]))
    worst = None
    for k, (a, b) in enumerate(zip(got[1], want[1])):
        if (a is None) != (b is None) or (a is not None and (a.shape != b.shape or a.dtype != b.dtype)):
            return "output %d: shape or type differs" % k
        if a is None or _bits(a) == _bits(b):       # (the same bits: np.array_equal, and a NaN equal to the same NaN)
            continue
        with np.errstate(invalid="ignore"):
            d = np.abs(a.astype(float) - b.astype(float))
        d = float(np.nanmax(d)) if np.any(np.isfinite(d)) else float("nan")
        if worst is None or not d <= worst[1]:
            raw = np.frombuffer(_bits(a), np.uint8).reshape(a.size, -1) != np.frombuffer(_bits(b), np.uint8).reshape(b.size, -1)
            at = np.flatnonzero(raw.any(axis=1))
            worst = (k, d, float(np.nanmax(np.abs(b.astype(float)))), at.size, a.size, int(at[0]), a.ravel()[at[0]], b.ravel()[at[0]])
    return None if worst is None else ("output %d differs from the fresh handle's: largest difference %.3e (largest entry %.3e), %d of "
                                       "%d entries, the first at %d: %r against %r" % worst)


def _run(monkeypatch, key, piece, first_index=0):
    """One piece of a circuit on one handle; returns (events compared, referees built for it, the model at the end)."""
    handle, streams, _ = PROBLEMS[key]
    kinds = SC.kinds_of(handle, streams)
    by_name = {k.name: k for k in kinds}
    calls = _calls(key)
    model = SC.Model(kinds)
    built = len(_REFEREES)
    fit = _fresh(monkeypatch, key)
    info = fit.krige_info if handle == "dense" else fit.krige_taper_info
    try:
        for i, name in enumerate(piece):
            ref = model.step(name)
            got = _event(fit, key, name, calls)
            want = _referee(monkeypatch, key, ref, calls, by_name)
            diff = _difference(got, want)
            assert diff is None, ("%s event %d, kind %s (held state: %s), behind %s: %s"
                                  % (key, first_index + i, name, ref.prepare, " <- ".join(reversed(piece[max(i - 3, 0):i])) or
                                     "nothing (a fresh handle)", diff))
            assert info()["prepared"] == (model.state is not None), (key, first_index + i, name, model.state)
        state = fit.engine_state()
        assert state["retries"] == 0, state
    finally:
        fit.close()
    return len(piece), len(_REFEREES) - built, model


def _circuit_part(monkeypatch, key, part):
    handle, streams, parts = PROBLEMS[key]
    kinds = SC.kinds_of(handle, streams)
    seq = SC.circuit(kinds, SC.SEEDS[handle])
    pieces = SC.split(seq, parts)
    first = sum(len(p) - 1 for p in pieces[:part])
    t0 = time.perf_counter()
    events, built, model = _run(monkeypatch, key, pieces[part], first)
    with_state, without, applies = SC.apply_shares(kinds, pieces[part])
    print("sequences-report | %s | part %d of %d | %d kinds, circuit of %d events | %d events compared here, 0 left out | %d "
          "bitwise kinds, %d by tolerance | %d referees built here (%d so far for this problem) | apply events %d, %.0f %% met a "
          "state | %.2f s" % (key, part + 1, parts, len(kinds), len(seq), events, len(kinds) - len(TOLERANCE), len(TOLERANCE),
                              built, sum(k[0] == key for k in _REFEREES), applies, 100 * with_state,
                              time.perf_counter() - t0))


@pytest.mark.parametrize("key,part", RUNS, ids=["%s-part%d" % kp for kp in RUNS])
def test_circuit(monkeypatch, key, part):
    """Part `part` of the problem's circuit on one handle, every event against its fresh-handle referee (module docstring)."""
    _circuit_part(monkeypatch, key, part)


# --------------------------------------------------------------------------- minimal sequences, by hand
def test_problems_have_the_layouts_they_are_chosen_for(monkeypatch):
    """n = 130: 126 rows of padding (placeholder observations in front, right-hand sides in slots behind); 256: no padding, tile
    rows under the matrix; 700: 68 rows of padding and the engine schedule (the objective's engine_state says so); the taper problems: unpacked, packed, irregular."""
    import ctypes
    T = SC.thetas(SC.dense_problem(130).theta)
    for n, pad, active in ((130, 126, False), (256, 0, False), (700, 68, True)):
        fit = _fresh(monkeypatch, "dense%d" % n)
        try:
            fit.neg2loglik_core(T["a"])
            assert fit.engine_state()["active"] == active, n
            lay = (ctypes.c_int * 5)()
            assert fit._L.cocons_debug_rhs_layout(fit._h, 0, lay) == 0
        finally:
            fit.close()
        # (out5 = pad0, nslot, ...: the placeholder observations in front and the slots behind fill the last tile)
        assert lay[0] + lay[1] == pad and (lay[1] > 0) == (pad > 0) and lay[0] >= 0, list(lay)
    for key, packed in (("taper_n129", False), ("taper_n640", True), ("taper_irregular", True)):
        prob = _problem(key)
        fit = _fresh(monkeypatch, key)
        try:
            nt, hi, W, pk = TE.envelope_of(prob.n, prob.ref_taper[0], prob.ref_taper[1], fit.order())
            info = fit.krige_taper_info()
        finally:
            fit.close()
        assert pk == packed and info["W"] == W and info["nt"] == nt, (key, info, W, nt)
        if key == "taper_irregular":
            assert not np.array_equal(hi, TE.floor_envelope(nt)) and not np.all(hi == nt), hi


@pytest.mark.parametrize("key", ["dense130", "dense700", "taper_n640"])
def test_failed_prepare_drops_the_state_and_a_failed_objective_keeps_it(monkeypatch, key):
    """prepare, failing objectives, apply: the held state's bits; then a failing prepare, apply: refused -- by hand, so that it
    does not hang on a seed."""
    handle = PROBLEMS[key][0]
    apply_, joint = [k.name for k in SC.kinds_of(handle) if k.role == "apply"]
    piece = ["prepare_b_z1", "value_npd", "value_nan", "batch3", apply_, joint, "prepare_a", "prepare_npd", apply_, joint,
             "release", "release", apply_]
    events, _, model = _run(monkeypatch, key, piece)
    assert events == len(piece) and model.state is None


# --------------------------------------------------------------------------- the caller's stream
def _job_accessors(monkeypatch):
    """cocons_fit_stream returns what was installed; cocons_fit_sync returns 0 and leaves the stream idle; an entry called while
    the caller's stream still holds queued torch work gives the own-stream bits; so does the NULL stream at n = 130; a batch on a
    caller's stream gives the fresh handle's values; destroying the handle leaves the caller's stream usable."""
    import torch
    key = "dense130"
    calls = _calls(key)
    ref = _fresh(monkeypatch, key)
    try:
        own = ref.stream()
        assert own != 0
        want = {k: _outcome(calls[k], ref) for k in ("value_a", "grad_a", "batch3", "predict300_b", "cv_folds_b")}
    finally:
        _close(ref)
    s = torch.cuda.Stream()
    fit = _fresh(monkeypatch, key)
    try:
        fit.set_stream(s.cuda_stream)
        assert fit.stream() == s.cuda_stream
        a = torch.randn(4096, 4096, device="cuda")
        with torch.cuda.stream(s):
            for _ in range(6):
                a = (a @ a) * 1e-3
        got = _outcome(calls["value_a"], fit)                  # (enqueued behind the products)
        assert _difference(got, want["value_a"]) is None
        for k in ("grad_a", "batch3", "predict300_b", "cv_folds_b"):
            assert _difference(_outcome(calls[k], fit), want[k]) is None, k
        assert fit._L.cocons_fit_sync(fit._h) == 0
        assert s.query(), "cocons_fit_sync left work on the stream"
        fit.set_stream(None)
        assert fit.stream() == 0
        for k in ("value_a", "grad_a", "batch3"):
            assert _difference(_outcome(calls[k], fit), want[k]) is None, "NULL stream, " + k
        fit.set_stream(s.cuda_stream)
        assert _difference(_outcome(calls["value_a"], fit), want["value_a"]) is None
        assert fit.engine_state()["retries"] == 0
    finally:
        fit.close()
    with torch.cuda.stream(s):
        b = torch.ones(1024, device="cuda").sum()
    s.synchronize()
    assert float(b) == 1024.0 and torch.isfinite(a).all()


def _job_six_streams(monkeypatch):
    """n = 700 (the engine schedule): six different caller's streams in turn, behind each the objective, the gradient and
    krige_prepare + krige_core.  cocons_fit_set_stream tests the handle's own pair against the new stream and redraws the
    library's engine stream on a clash, so no engine hand-off times out (retries == 0; this test is not marked shared_gpu).
    Where the operation ran on the engine schedule its values equal the own-stream handle's bit for bit; where the handle
    has left the engine (no clash-free draw) they agree within the 1e-12 relative that test_batch_matches_single_calls grants
    the plain schedule against the engine schedule."""
    import torch
    key = "dense700"
    calls = _calls(key)
    names = ("value_a", "grad_a", "prepare_a", "krige70")
    ref = _fresh(monkeypatch, key)
    try:
        want = {k: _outcome(calls[k], ref) for k in names}
        assert ref.engine_state()["active"]
    finally:
        _close(ref)
    assert all(w[0] == "ok" for w in want.values())
    streams = [torch.cuda.Stream() for _ in range(6)]
    stayed = []
    fit = _fresh(monkeypatch, key)
    try:
        for j, s in enumerate(streams):
            fit.set_stream(s.cuda_stream)
            assert fit.stream() == s.cuda_stream
            on_engine = True
            for k in names:
                got = _outcome(calls[k], fit)
                state = fit.engine_state()
                assert state["retries"] == 0, (j, k, state)
                if k != "krige70":                         # (apply factors nothing: it reads the factor prepare left)
                    active = state["active"]
                on_engine = on_engine and active
                assert got[0] == "ok", (j, k, got)
                if active:
                    assert _difference(got, want[k]) is None, (j, k, _difference(got, want[k]))
                else:
                    for a, b in zip(got[1], want[k][1]):
                        assert np.allclose(a, b, rtol=1e-12, atol=0), (j, k)
            stayed.append(on_engine)
            assert s.query() or fit._L.cocons_fit_sync(fit._h) == 0
    finally:
        fit.close()
    print("sequences-report | dense700 | six caller's streams, engine stayed active: %s" % ["yes" if x else "no" for x in stayed])


# --------------------------------------------------------------------------- the child process that imports torch first
JOBS = ["circuit:%s:%d" % kp for kp in STREAM_RUNS] + ["accessors", "six_streams"]


def _run_job(job, monkeypatch):
    if job.startswith("circuit:"):
        _, key, part = job.split(":")
        _circuit_part(monkeypatch, key, int(part))
    else:
        {"accessors": _job_accessors, "six_streams": _job_six_streams}[job](monkeypatch)


def _child_main(out_path, jobs=()):
    """every job (or the named ones) in turn, each with a MonkeyPatch of its own; {job: [passed, seconds, text]} as JSON.  A job that ends in anything
    but a failed assertion (a HIP error, say) ends the child: nothing more is started on the GPU behind it."""
    import contextlib
    import io
    import json
    import traceback
    import torch                      # BEFORE the library is loaded: its HIP runtime is the process's (module docstring)
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    results = {}
    for job in (jobs or JOBS):
        mp = pytest.MonkeyPatch()
        text = io.StringIO()
        t0 = time.perf_counter()
        stop = False
        try:
            with contextlib.redirect_stdout(text):
                _run_job(job, mp)
            passed = True
        except AssertionError:
            passed = False
            text.write(traceback.format_exc())
        except BaseException:
            passed, stop = False, True
            text.write(traceback.format_exc())
        finally:
            mp.undo()
        results[job] = [passed, time.perf_counter() - t0, text.getvalue()]
        with open(out_path, "w") as fh:
            json.dump(results, fh)
        if stop:
            break


@pytest.fixture(scope="module")
def torch_jobs(tmp_path_factory):
    """the child process, once: {job: [passed, seconds, text]}"""
    import json
    import subprocess
    out = str(tmp_path_factory.mktemp("sequences") / "jobs.json")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=900)
    results = {}
    if os.path.exists(out):
        with open(out) as fh:
            results = json.load(fh)
    return proc.returncode, proc.stdout, results


def _reported(torch_jobs, job):
    rc, output, results = torch_jobs
    assert job in results, "the child process ended (exit status %d) before job %s:\n%s" % (rc, job, output[-4000:])
    passed, seconds, text = results[job]
    print(text.rstrip())
    print("sequences-report | job %s | %.2f s in the child process" % (job, seconds))
    assert passed, text


@pytest.mark.parametrize("key,part", STREAM_RUNS, ids=["%s-part%d" % kp for kp in STREAM_RUNS])
def test_circuit_with_callers_streams(torch_jobs, key, part):
    """the circuits of the plain-schedule handles with the two "install a caller's stream" kinds: everything behind them equals
    the fresh own-stream referee bit for bit (_circuit_part in the child process)"""
    _reported(torch_jobs, "circuit:%s:%d" % (key, part))


def test_stream_accessors_and_queued_work(torch_jobs):
    """_job_accessors in the child process"""
    _reported(torch_jobs, "accessors")


def test_engine_size_handle_on_six_callers_streams(torch_jobs):
    """_job_six_streams in the child process"""
    _reported(torch_jobs, "six_streams")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child_main(sys.argv[1], sys.argv[2:])
