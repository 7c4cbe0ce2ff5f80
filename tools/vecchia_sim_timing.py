"""Time U^-1 on a Vecchia fit: python tools/vecchia_sim_timing.py [n ...] [--m 30] [--sorted-up-to 100000] [--out FILE].

The setting of tools/vecchia_knn_timing.py: for every n (default 10000 99856 1000000) uniform sites on the unit square in random
order (the Vecchia order) and, for n up to --sorted-up-to, the same sites sorted by x (an adversarial order: a deep dependency
graph); the design and theta of tools/taper_timing.py, the m nearest earlier rows found on the device
(CoconsVecchiaFit.from_knn).  Timed with the host clock around calls that end in a device synchronise (every entry drains its
stream before it returns), the smallest and the median of several calls after a warm-up, the two settings of
COCONS_VECCHIA_SIM_FUSE in alternation (the library reads the switch at every call):
  - cocons_vecchia_schedule on a fresh handle: depth, rows of the largest level, launches of one solve with and without fused
    runs, device bytes;
  - cocons_vecchia_unwhiten with c = 1 and c = 16 columns, host copies included;
  - its split by events on the device (cocons_debug_vecchia_sim_phases): the coefficients, the schedule (first call of a
    handle only) and the solve;
  - whether the two settings give the same bits;
  - beside them, as yardsticks only: cocons_neg2loglik_vecchia on the same handle (the cost of the coefficient phase), and at
    n <= 10000 cocons_sim_dense with one column (a different model).
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
SORTED_UP_TO = int(_opt("--sorted-up-to", 100000))
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
SWITCH = "COCONS_VECCHIA_SIM_FUSE"
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def fuse(on):
    os.environ[SWITCH] = "1" if on else "0"


def timed_pair(fn, reps):
    """(min, median) ms of fn with fused runs, then without: the two settings in alternation after a warm-up of each"""
    ts = {True: [], False: []}
    for on in (True, False):
        fuse(on)
        fn()
    for _ in range(reps):
        for on in (True, False):
            fuse(on)
            t0 = time.perf_counter()
            fn()
            ts[on].append(time.perf_counter() - t0)
    fuse(True)
    return tuple((1e3 * min(ts[on]), 1e3 * float(np.median(ts[on]))) for on in (True, False))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts))


def phases(fit, th, W):
    """(ms coefficients, ms schedule, ms solve) of one cocons_vecchia_unwhiten, by events on the handle's stream"""
    T = host.theta_table(th)
    out, ms = np.zeros(W.shape, order="F"), np.zeros(3)
    _lib.check(fit._L.cocons_debug_vecchia_sim_phases(fit._h, host._p(T), int(W.shape[1]), host._p(W), host._p(out), host._p(ms)),
               "cocons_debug_vecchia_sim_phases")
    return ms


th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_sim_timing.py %s --m %d --sorted-up-to %d" % (" ".join(map(str, SIZES)), M, SORTED_UP_TO))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    sites = rng.uniform(0, 1, size=(n, 2))
    reps = 10 if n <= 100000 else 5
    for order in ("random", "sorted by x"):
        if order != "random" and n > SORTED_UP_TO:
            continue
        locs = sites if order == "random" else sites[np.argsort(sites[:, 0], kind="stable")]
        sc = wl.design_from_locs(locs)
        X, z = sc["std.covs"], wl.synthetic_z(n)
        W = np.asfortranarray(np.random.default_rng(n + 1).standard_normal((n, 16)))
        W1 = np.asfortranarray(W[:, :1])
        fit = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, M)
        fuse(True)
        t0 = time.perf_counter()
        first = phases(fit, th, W1)                       # the handle's first call: the schedule is made in it
        t_first = 1e3 * (time.perf_counter() - t0)
        s_on = fit.schedule()
        fuse(False)
        s_off = fit.schedule()
        fuse(True)
        sizes = np.bincount(s_on["levels"])[1:]
        say("n = %d, m = %d, %s order: depth %d, largest level %d rows, median level %d rows, %d levels of at most 256 rows; "
            "launches of one solve %d with fused runs, %d without; schedule and coefficients %.1f MB on the device" %
            (n, M, order, s_on["depth"], s_on["widest"], int(np.median(sizes)), int(np.count_nonzero(sizes <= 256)),
             s_on["launches"], s_off["launches"], s_on["bytes"] / 1e6))
        say("  first call of the handle (c = 1) %10.3f ms by the host clock; by events: coefficients %.3f ms, schedule %.3f ms, "
            "solve %.3f ms" % (t_first, first[0], first[1], first[2]))
        for c, Wc in ((1, W1), (16, W)):
            (on, off) = timed_pair(lambda: fit.unwhiten_core(th, Wc), reps)
            fuse(True)
            a = fit.unwhiten_core(th, Wc)
            p_on = min((phases(fit, th, Wc) for _ in range(reps)), key=lambda v: v.sum())
            fuse(False)
            b = fit.unwhiten_core(th, Wc)
            p_off = min((phases(fit, th, Wc) for _ in range(reps)), key=lambda v: v.sum())
            fuse(True)
            say("  cocons_vecchia_unwhiten c = %-2d   fused runs %10.3f ms (median %10.3f), one launch per level %10.3f ms (median "
                "%10.3f) over %d calls each, alternating, host copies included; same bits: %s" %
                ((c,) + on + off + (reps, bool(np.array_equal(a, b)))))
            say("    by events (the call of %d with the smallest sum): coefficients %.3f ms, solve %.3f ms with fused runs; "
                "coefficients %.3f ms, solve %.3f ms with one launch per level" % (reps, p_on[0], p_on[2], p_off[0], p_off[2]))
        t_val = timed(lambda: fit.neg2loglik_core(th), reps)
        say("  cocons_neg2loglik_vecchia        %10.3f ms (median %10.3f): the yardstick of the coefficient phase" % t_val)
        if n <= 10000 and order == "random":
            d = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
            t_dense = timed(lambda: d.sim_core(th, W1), 3)
            d.close()
            say("  cocons_sim_dense, one column     %10.3f ms (median %10.3f): a different model, a yardstick only" % t_dense)
        fit.close()
os.environ.pop(SWITCH, None)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
