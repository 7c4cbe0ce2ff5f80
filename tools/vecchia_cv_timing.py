"""Time U' and cross-validation on a Vecchia fit: python tools/vecchia_cv_timing.py [n ...] [--m 30] [--star 1000000] [--out FILE].

The README's setting, as tools/vecchia_sim_timing.py has it: for every n (default 10000 99856 1000000) uniform sites on the unit
square in random order and in the maxmin order (CoconsVecchiaFit.from_maxmin), the design and theta of tools/taper_timing.py
(the Bessel branch), the m nearest earlier rows found on the device.  Timed with the host clock around calls that end in a
device synchronise (every entry drains its stream before it returns), the smallest and the median of several calls after a
warm-up; the build's phases by events on the handle's stream (cocons_debug_vecchia_transpose_phases):
  - the transposed lists, once per handle: counts / scan / fill / sort (with the places), entries, longest list, and the
    handle's device bytes before and after;
  - cocons_cv_vecchia leave-one-out with r = 1 and r = 4 realisations, by random folds of 10 (n / 10 folds) and of 128;
  - cocons_vecchia_whiten_t of 1 and 16 columns;
  - beside them, of the same visit and the same handle: cocons_neg2loglik_vecchia (a value call) and the coefficient launch
    (the first phase of cocons_debug_vecchia_sim_phases) -- the parent's entries and the only baseline; each ratio is to the
    value call's smallest time;
  - once, the build alone on the adversarial star (every row names row 1) at --star rows (0: not run).
Nothing is asserted; the lines also go to --out."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca                     # noqa: E402
from cocons_amd import _lib, host, workloads as wl      # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


M = int(_opt("--m", 30))
STAR = int(_opt("--star", 1000000))
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts))


def build_phases(fit):
    ms = np.zeros(4)
    _lib.check(fit._L.cocons_debug_vecchia_transpose_phases(fit._h, host._p(ms)), "cocons_debug_vecchia_transpose_phases")
    return ms


def coef_ms(fit, th, reps):
    """device ms of the coefficient launch: the first phase of cocons_debug_vecchia_sim_phases, the smallest of reps calls"""
    T = host.theta_table(th)
    W = np.zeros((fit.n, 1), order="F")
    out, ms, best = np.zeros(W.shape, order="F"), np.zeros(3), np.inf
    for _ in range(reps + 1):
        _lib.check(fit._L.cocons_debug_vecchia_sim_phases(fit._h, host._p(T), 1, host._p(W), host._p(out), host._p(ms)),
                   "cocons_debug_vecchia_sim_phases")
        best = min(best, float(ms[0]))
    return best


th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_cv_timing.py %s --m %d --star %d" % (" ".join(map(str, SIZES)), M, STAR))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    X = wl.design_from_locs(locs)["std.covs"]
    z4 = np.asfortranarray(np.random.default_rng(n + 2).standard_normal((n, 4)))
    W = np.asfortranarray(np.random.default_rng(n + 1).standard_normal((n, 16)))
    W1 = np.asfortranarray(W[:, :1])
    reps = 10 if n <= 100000 else 3
    perm = np.random.default_rng(n + 3).permutation(n)
    folds = {10: (perm // 10).astype(np.int32), 128: (perm // 128).astype(np.int32)}
    for order in ("random", "maxmin"):
        make = ca.CoconsVecchiaFit.from_knn if order == "random" else ca.CoconsVecchiaFit.from_maxmin
        fit = make(locs, X, z4[:, :1], wl.SMOOTH_LIMITS, M)
        fit4 = make(locs, X, z4, wl.SMOOTH_LIMITS, M)
        before = fit.info()["bytes"]
        t0 = time.perf_counter()
        t = fit.transpose()
        t_first = 1e3 * (time.perf_counter() - t0)
        ph = min((build_phases(fit) for _ in range(3)), key=lambda v: v.sum())
        lens = np.diff(t["ptr"])
        say("n = %d, m = %d, %s order: %d entries, longest list %d, mean %.1f, %d columns nobody names, %d lists above 64 rows; "
            "lists %.1f MB on the device" % (n, M, order, t["entries"], t["longest"], lens.mean(), t["unnamed"],
                                            int(np.sum(lens > 64)), t["bytes"] / 1e6))
        say("  transposed lists, once per handle: first call %10.3f ms by the host clock (the lists come home in it); by events, "
            "the build of 3 with the smallest sum: count %.3f ms, scan %.3f ms, fill %.3f ms, sort and places %.3f ms, together "
            "%.3f ms" % (t_first, ph[0], ph[1], ph[2], ph[3], ph.sum()))
        t_val = timed(lambda: fit.neg2loglik_core(th), reps)
        t_val4 = timed(lambda: fit4.neg2loglik_core(th), reps)
        c_ms = coef_ms(fit, th, reps)
        say("  cocons_neg2loglik_vecchia r = 1   %10.3f ms (median %10.3f), r = 4 %10.3f ms (median %10.3f); the coefficient "
            "launch %.3f ms by events: the baseline of this visit" % (t_val + t_val4 + (c_ms,)))
        rows = [("leave-one-out, r = 1", lambda: fit.cv_core(th)), ("leave-one-out, r = 4", lambda: fit4.cv_core(th))]
        for b, lab in folds.items():
            rows.append(("folds of %d (%d folds), r = 1" % (b, int(lab.max()) + 1), lambda lab=lab: fit.cv_core(th, lab)))
        rows += [("whiten_t, c = 1", lambda: fit.whiten_t_core(th, W1)), ("whiten_t, c = 16", lambda: fit.whiten_t_core(th, W))]
        for name, fn in rows:
            lo, med = timed(fn, reps)
            say("  %-36s %10.3f ms (median %10.3f) over %d calls, host copies included: %.2f value calls" %
                (name, lo, med, reps, lo / t_val[0]))
        st = fit.cv_core(th, folds[10], stats=True)[2]
        after = fit.info()["bytes"]
        say("  device bytes of the handle: %.1f MB before the first of these calls, %.1f MB after (lists %.1f MB, coefficients "
            "%.1f MB); a call by folds of 10 allocates %.1f MB beside them" %
            (before / 1e6, after / 1e6, t["bytes"] / 1e6, n * (M + 1) * 8 / 1e6, st["bytes"] / 1e6))
        fit.close()
        fit4.close()
if STAR > 0:
    n = STAR
    rng = np.random.default_rng(7)
    locs = rng.uniform(0, 1, size=(n, 2))
    nn = np.ones((n, 1), dtype=np.int32, order="F")
    nn[0, 0] = 0
    fit = ca.CoconsVecchiaFit(locs, np.asfortranarray(np.column_stack([np.ones(n), locs])), np.zeros(n), wl.SMOOTH_LIMITS, nn)
    t0 = time.perf_counter()
    ph = build_phases(fit)
    t_host = 1e3 * (time.perf_counter() - t0)
    t = fit.transpose()
    ok = bool(np.array_equal(t["rows"], np.arange(2, n + 1)))
    say("star, n = %d, m = 1 (every row names row 1: one list of %d rows, sorted in memory by one workgroup), the build alone, "
        "once: %.3f ms by the host clock; by events count %.3f ms, scan %.3f ms, fill %.3f ms, sort and places %.3f ms; the "
        "list is 2 .. n: %s" % (n, t["longest"], t_host, ph[0], ph[1], ph[2], ph[3], ok))
    fit.close()
