"""Time the maxmin ordering on the device: python tools/vecchia_order_timing.py [n ...] [--m 30] [--host-max 1000000] [--out FILE].

The setting of tools/vecchia_timing.py: for every n (default 10000 99856 1000000) uniform sites on the unit square in random
order, the design and theta of tools/taper_timing.py.  Timed with the host clock around calls that end in a device synchronise,
the smallest, the median and the largest of several calls after a warm-up:
  - cocons_vecchia_order (upload of the sites, the levels, download of the order), its split by events on the device and its
    work -- levels, rounds, launches, host reads of a counter -- (cocons_debug_order_phases);
  - host.vecchia_order, the same rule on the host, ONCE IN THE SAME VISIT for n up to --host-max, and whether its order is the
    device's;
  - the same call for the sites sorted by x (n up to 100000);
  - what the order buys downstream: depth of the level schedule of U^-1 and the time of one simulated field
    (cocons_sim_vecchia) and of one value, for the handle on the sites as they come (a random order) and on the maxmin order;
  - at n = 4096, for one field drawn from the dense model: the Vecchia value's distance from the dense value for the random
    order and for the maxmin order.
Nothing is asserted; the lines also go to --out."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca                     # noqa: E402
from cocons_amd import _lib, workloads as wl      # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


M = int(_opt("--m", 30))
HOST_MAX = int(_opt("--host-max", 1000000))
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps):
    fn()                                     # warm-up: code objects, first allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts)), 1e3 * max(ts)


def phases(locs):
    """(ms4, stats5) of one ordering, by events on the device"""
    L = _lib.load()
    f = np.asfortranarray(locs, dtype=np.float64)
    ms, st = np.zeros(4), np.zeros(5, dtype=np.int64)
    _lib.check(L.cocons_debug_order_phases(f.shape[0], f.ctypes.data_as(_lib.c_dp), 0, 0, None, None, ms.ctypes.data_as(_lib.c_dp),
                                           st.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))), "cocons_debug_order_phases")
    return ms, st


def order_lines(what, locs, reps, host):
    n = locs.shape[0]
    order, counts = ca.vecchia_order_device(locs, levels=True)
    t = timed(lambda: ca.vecchia_order_device(locs), reps)
    phases(locs)
    ms, st = min((phases(locs) for _ in range(reps)), key=lambda v: v[0].sum())
    say("n = %d, %s: level sizes %s" % (n, what, counts.tolist()))
    say("  cocons_vecchia_order             %10.3f ms (median %10.3f, largest %10.3f) over %d calls, upload and the order's download "
        "included" % (t + (reps,)))
    say("    by events on the device (the call of %d with the smallest sum): relabel %.3f ms, dense levels %.3f ms, binned levels "
        "%.3f ms, the levels' ends %.3f ms; %d levels, %d of them dense, %d rounds, %d launches, %d host reads" %
        ((reps,) + tuple(ms) + tuple(int(v) for v in st)))
    if host:
        t0 = time.perf_counter()
        o_host = ca.vecchia_order(locs)
        t_host = time.perf_counter() - t0
        say("  host.vecchia_order               %10.1f ms, once, in the same visit: %.1f times the device call; the same order: %s" %
            (1e3 * t_host, 1e3 * t_host / t[0], bool(np.array_equal(o_host, order))))
    else:
        say("  host.vecchia_order               not run at this size")
    return order


th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_order_timing.py %s --m %d --host-max %d" % (" ".join(map(str, SIZES)), M, HOST_MAX))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    reps = 10 if n <= 100000 else 5
    order = order_lines("uniform sites in random order", locs, reps, n <= HOST_MAX)
    if n <= 100000 and n > 50000:
        order_lines("the same sites sorted by x", locs[np.argsort(locs[:, 0], kind="stable")], reps, False)
    o = order.astype(np.int64) - 1
    E = np.asfortranarray(np.random.default_rng(n + 1).standard_normal((n, 1)))
    for what, l in (("random order", locs), ("maxmin order", locs[o])):
        sc = wl.design_from_locs(l)
        X, z = sc["std.covs"], wl.synthetic_z(n)
        fit = ca.CoconsVecchiaFit.from_knn(l, X, z, wl.SMOOTH_LIMITS, M)
        fit.sim_core(th, E)
        s = fit.schedule()
        t_sim = timed(lambda: fit.sim_core(th, E), reps)
        t_val = timed(lambda: fit.neg2loglik_core(th), reps)
        say("  downstream, %s: schedule of U^-1 depth %d, widest level %d rows, %d launches; cocons_sim_vecchia, one field %10.3f ms "
            "(median %10.3f); cocons_neg2loglik_vecchia %10.3f ms (median %10.3f)" %
            (what, s["depth"], s["widest"], s["launches"], t_sim[0], t_sim[1], t_val[0], t_val[1]))
        fit.close()

# the value's distance from the dense value, n = 4096
n = 4096
rng = np.random.default_rng(20260000 + n)
locs = rng.uniform(0, 1, size=(n, 2))
sc = wl.design_from_locs(locs)
X = sc["std.covs"]
d = ca.CoconsFit(locs, X, np.zeros(n), wl.SMOOTH_LIMITS)
z = d.sim_core(th, np.random.default_rng(n + 1).standard_normal((n, 1)))      # one field of the dense model itself
d.close()
d = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
dense = d.neg2loglik_core(th)[0]
d.close()
a = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, M)
b = ca.CoconsVecchiaFit.from_maxmin(locs, X, z, wl.SMOOTH_LIMITS, M)
va, vb = a.neg2loglik_core(th)[0], b.neg2loglik_core(th)[0]
a.close()
b.close()
say("n = %d, m = %d, -2 log-likelihood: dense %.6f; Vecchia in random order %.6f (off by %.4f), in maxmin order %.6f (off by %.4f)" %
    (n, M, dense, va, va - dense, vb, vb - dense))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
