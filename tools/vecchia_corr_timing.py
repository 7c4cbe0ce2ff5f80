"""Time the Vecchia neighbours by model correlation on the device: python tools/vecchia_corr_timing.py [n ...] [--m 30] [--out FILE].

The setting of tools/vecchia_knn_timing.py: for every n (default 10000 99856 1000000) uniform sites on the unit square, in
random order (as they come) and in the maxmin order of cocons_vecchia_order, the design and theta of tools/taper_timing.py (the
Bessel branch), m neighbours.  Timed with the host clock around calls that end in a device synchronise (every entry drains its
stream before it returns): the smallest, the median and the largest of several calls after a warm-up.  For (m_cand, hops) =
(60, 1), (30, 2), (60, 2):
  - CoconsVecchiaFit.neighbours_corr (the search of width m_cand, the records at theta, the re-ranking, the n x m table's
    download), and its three phases by events on the device (cocons_debug_knn_corr_phases; the call with the smallest sum);
  - the mean number of unique candidates a row ranks -- what the re-ranking's cost scales with --, counted on the host from
    the Euclidean table over a sample of rows;
  - CoconsVecchiaFit.from_corr_knn (neither table leaves the device);
and beside them, from the same visit: cocons_vecchia_neighbours at m, CoconsVecchiaFit.from_knn, and one value call
(neg2loglik_core) on the handle.  Nothing is asserted; the lines also go to --out."""
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
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
SETTINGS = ((60, 1), (30, 2), (60, 2))
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


def phases(fit, T, mc, hops):
    ms = np.zeros(3)
    _lib.check(fit._L.cocons_debug_knn_corr_phases(fit._h, T.ctypes.data_as(_lib.c_dp), mc, hops, M, ms.ctypes.data_as(_lib.c_dp)),
               "cocons_debug_knn_corr_phases")
    return ms


def unique_candidates(cand, hops, rows):
    total = 0
    for i in rows:
        c = cand[i][cand[i] > 0]
        if hops == 2 and c.size:
            c = np.concatenate([c, cand[c - 1].ravel()])
        total += np.unique(c[c > 0]).size
    return total / len(rows)


th = wl.theta_full()
th["mean"] = np.zeros(3)
T = host.theta_table(th)
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_corr_timing.py %s --m %d" % (" ".join(map(str, SIZES)), M))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    locs0 = rng.uniform(0, 1, size=(n, 2))
    X0, z0 = wl.design_from_locs(locs0)["std.covs"], wl.synthetic_z(n)
    reps = 10 if n <= 100000 else 5
    sample = np.sort(rng.choice(n, size=min(n, 2000), replace=False))
    for oname in ("random order", "maxmin order"):
        o = np.arange(n) if oname == "random order" else ca.vecchia_order_device(locs0).astype(np.int64) - 1
        locs, X, z = np.ascontiguousarray(locs0[o]), np.asfortranarray(X0[o]), z0[o]
        fit = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, M)
        t_nn = timed(lambda: ca.vecchia_neighbours_device(locs, M), reps)
        t_val = timed(lambda: fit.neg2loglik_core(th), reps)
        t_knn = timed(lambda: ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, M).close(), max(reps // 2, 3))
        say("n = %d, m = %d, %s (min / median / max of %d calls, ms)" % (n, M, oname, reps))
        say("  cocons_vecchia_neighbours at m   %10.3f / %10.3f / %10.3f" % t_nn)
        say("  one value call (neg2loglik_core) %10.3f / %10.3f / %10.3f" % t_val)
        say("  CoconsVecchiaFit.from_knn        %10.3f / %10.3f / %10.3f" % t_knn)
        for mc, hops in SETTINGS:
            cand = ca.vecchia_neighbours_device(locs, mc)
            uniq = unique_candidates(cand, hops, sample)
            t_call = timed(lambda: fit.neighbours_corr(th, M, m_cand=mc, hops=hops), reps)
            phases(fit, T, mc, hops)
            ph = min((phases(fit, T, mc, hops) for _ in range(reps)), key=lambda v: v.sum())
            t_fit = timed(lambda: ca.CoconsVecchiaFit.from_corr_knn(locs, X, z, wl.SMOOTH_LIMITS, th, M, m_cand=mc, hops=hops).close(),
                          max(reps // 2, 3))
            say("  m_cand = %d, hops = %d: %.1f unique candidates a row (mean over %d rows)" % (mc, hops, uniq, len(sample)))
            say("    neighbours_corr                %10.3f / %10.3f / %10.3f = %.2f value calls" % (t_call + (t_call[0] / t_val[0],)))
            say("      by events on the device: the search %.3f ms, the records %.3f ms, the re-ranking kernel %.3f ms = %.2f value "
                "calls; the rest of the call is allocations, the table's download and the host" % (ph[0], ph[1], ph[2], ph[2] / t_val[0]))
            say("    CoconsVecchiaFit.from_corr_knn %10.3f / %10.3f / %10.3f = %.2f of from_knn" % (t_fit + (t_fit[0] / t_knn[0],)))
        fit.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
