"""Time local kriging on correlation-ranked neighbours and the grouped handle on a correlation table on the device:
python tools/vecchia_corr_pred_timing.py [n ...] [--m 30] [--mp 100000] [--out FILE].

The setting of tools/vecchia_corr_timing.py: for every n (default 10000 99856 1000000) uniform sites on the unit square as
they come, the design and theta of tools/taper_timing.py (the Bessel branch), m neighbours, mp uniform new sites.  Timed with
the host clock around calls that end in a device synchronise (every entry drains its stream before it returns): the smallest,
the median and the largest of several calls after a warm-up.
  - predict_knn_core at m (cocons_vecchia_predict_knn), and for (m_cand, hops) = (60, 1), (30, 2), (60, 2)
    predict_corr_knn_core and neighbours_corr_pred; the difference of the smallest times of predict_corr_knn_core and
    predict_knn_core is the wider query, the re-ranking launch and one more drain per chunk together (the launch alone is
    not split out: no entry records events around it);
  - the one-off build of the all-observations table: the first call with two hops at a width against the later ones, and the
    bytes cocons_vecchia_info gains;
  - from_groups_corr_knn against the host route (neighbours_corr -> vecchia_group_rounds -> vecchia_group_table -> the
    constructor -> set_groups) and against from_groups_knn.
Nothing is asserted; the lines also go to --out."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca                     # noqa: E402
from cocons_amd import host, workloads as wl      # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


M = int(_opt("--m", 30))
MP = int(_opt("--mp", 100000))
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
SETTINGS = ((60, 1), (30, 2), (60, 2))
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps, warm=True):
    if warm:
        fn()                                 # warm-up: code objects, first allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts)), 1e3 * max(ts)


def host_route(locs, X, z, th, mc, hops, cap=64):
    f0 = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, 1)
    nn = f0.neighbours_corr(th, M, m_cand=mc, hops=hops)
    f0.close()
    group = host.vecchia_group_rounds(nn, cap)
    g = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, host.vecchia_group_table(nn, group))
    g.set_groups(group)
    g.close()


th = wl.theta_full()
th["mean"] = np.zeros(3)
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_corr_pred_timing.py %s --m %d --mp %d" % (" ".join(map(str, SIZES)), M, MP))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    sc = wl.design_from_locs(locs)
    X, z = np.asfortranarray(sc["std.covs"]), wl.synthetic_z(n)
    lp = np.asfortranarray(rng.uniform(0, 1, size=(MP, 2)))
    Xp = np.asfortranarray(wl.design_from_locs(lp, sc["mean.vector"], sc["sd.vector"])["std.covs"])
    reps = 20 if n <= 100000 else 10
    fit = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, M)
    t_knn = timed(lambda: fit.predict_knn_core(th, lp, Xp, M), reps)
    say("n = %d, m = %d, %d new sites (min / median / max of %d calls, ms)" % (n, M, MP, reps))
    say("  predict_knn_core                  %10.3f / %10.3f / %10.3f" % t_knn)
    for mc, hops in SETTINGS:
        b0 = fit.info()["bytes"]
        t0 = time.perf_counter()
        fit.predict_corr_knn_core(th, lp, Xp, M, m_cand=mc, hops=hops)
        first = 1e3 * (time.perf_counter() - t0)
        grown = fit.info()["bytes"] - b0
        t_pred = timed(lambda: fit.predict_corr_knn_core(th, lp, Xp, M, m_cand=mc, hops=hops), reps, warm=False)
        t_tab = timed(lambda: fit.neighbours_corr_pred(th, lp, Xp, M, m_cand=mc, hops=hops), reps)
        say("  m_cand = %d, hops = %d" % (mc, hops))
        say("    predict_corr_knn_core           %10.3f / %10.3f / %10.3f = %.2f of predict_knn_core; over it %.3f ms (wider query, "
            "re-ranking, a drain per chunk)" % (t_pred + (t_pred[0] / t_knn[0], t_pred[0] - t_knn[0])))
        say("    neighbours_corr_pred            %10.3f / %10.3f / %10.3f" % t_tab)
        say("    first call at this width %.3f ms, %.3f ms over the smallest later one; the handle grew by %d bytes"
            % (first, first - t_pred[0], grown))
    fit.close()
    reps_h = 5 if n <= 100000 else 3
    t_gk = timed(lambda: ca.CoconsVecchiaFit.from_groups_knn(locs, X, z, wl.SMOOTH_LIMITS, M).close(), reps_h)
    say("  from_groups_knn                   %10.3f / %10.3f / %10.3f" % t_gk)
    for mc, hops in SETTINGS:
        t_dev = timed(lambda: ca.CoconsVecchiaFit.from_groups_corr_knn(locs, X, z, wl.SMOOTH_LIMITS, th, M, m_cand=mc, hops=hops).close(),
                      reps_h)
        t_host = timed(lambda: host_route(locs, X, z, th, mc, hops), 2, warm=False)
        say("  m_cand = %d, hops = %d: from_groups_corr_knn %10.3f / %10.3f / %10.3f = %.2f of from_groups_knn; the host route "
            "%.3f / %.3f / %.3f (2 calls)" % ((mc, hops) + t_dev + (t_dev[0] / t_gk[0],) + t_host))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
