"""Time the Vecchia neighbour search on the device: python tools/vecchia_knn_timing.py [n ...] [--m 30] [--pred 100000] [--out FILE].

The setting of tools/vecchia_timing.py: for every n (default 10000 99856 1000000) uniform sites on the unit square in random
order (the Vecchia order), the design and theta of tools/taper_timing.py, m neighbours.  Timed with the host clock around calls
that end in a device synchronise (every entry drains its stream before it returns), the smallest and the median of several
calls after a warm-up:
  - cocons_vecchia_neighbours (upload of the sites, the search, download of the n x m table), and the split of the search
    between binning the levels and the queries by events on the device (cocons_debug_knn_phases);
  - CoconsVecchiaFit.from_knn (the table never leaves the device) beside CoconsVecchiaFit from a table that is already there;
  - host.vecchia_neighbours, the k-d trees on the host, ONCE IN THE SAME VISIT (it takes seconds), and whether its table is
    the device's;
  - `--pred` predictions: predict_knn_core, against host.vecchia_neighbours_pred (the k-d tree query) followed by predict_core
    with its table.  predict_core is the path of cocons_vecchia_predict as it was before the search existed: its time is
    the baseline;
  - the device bytes the handle holds before and after the first predict_knn_core call (the grid over the observations).
Nothing is asserted; the lines also go to --out."""
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
NPRED = int(_opt("--pred", 100000))
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
    return 1e3 * min(ts), 1e3 * float(np.median(ts))


def phases(locs):
    """(ms binning the levels, ms of the query launches) of one ordered self search, by events on the device"""
    L = _lib.load()
    f = np.asfortranarray(locs, dtype=np.float64)
    ms = np.zeros(2)
    _lib.check(L.cocons_debug_knn_phases(f.shape[0], f.ctypes.data_as(_lib.c_dp), M, 0, ms.ctypes.data_as(_lib.c_dp)),
               "cocons_debug_knn_phases")
    return ms


th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_knn_timing.py %s --m %d --pred %d" % (" ".join(map(str, SIZES)), M, NPRED))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    sc = wl.design_from_locs(locs)
    X, z = sc["std.covs"], wl.synthetic_z(n)
    new = rng.uniform(0, 1, size=(max(NPRED, 1), 2))
    Xn = wl.design_from_locs(new, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    reps = 10 if n <= 100000 else 5
    nn = ca.vecchia_neighbours_device(locs, M)
    t_dev = timed(lambda: ca.vecchia_neighbours_device(locs, M), reps)
    phases(locs)
    ph = min((phases(locs) for _ in range(reps)), key=lambda v: v.sum())
    t0 = time.perf_counter()
    nn_host = ca.vecchia_neighbours(locs, M)
    t_host = time.perf_counter() - t0

    def from_knn():
        ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, M).close()

    def from_table():
        ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn).close()

    t_knn = timed(from_knn, max(reps // 2, 3))
    fit = ca.CoconsVecchiaFit.from_knn(locs, X, z, wl.SMOOTH_LIMITS, M)
    t_tab = timed(from_table, max(reps // 2, 3))
    say("n = %d, m = %d: rows where the device's table differs from host.vecchia_neighbours': %d" %
        (n, M, int(np.count_nonzero(np.any(nn != nn_host, axis=1)))))
    say("  cocons_vecchia_neighbours        %10.3f ms (median %10.3f) over %d calls, upload and the n x m table's download included" %
        (t_dev + (reps,)))
    say("    by events on the device: binning the levels %.3f ms, the queries %.3f ms (the call of %d with the smallest sum); the "
        "rest of the call is allocations, the upload, the table's download and the host" % (ph[0], ph[1], reps))
    say("  host.vecchia_neighbours          %10.1f ms, once, in the same visit: %.1f times the device call" %
        (1e3 * t_host, 1e3 * t_host / t_dev[0]))
    say("  CoconsVecchiaFit.from_knn        %10.3f ms (median %10.3f); CoconsVecchiaFit from a ready table %.3f ms (median %.3f)" %
        (t_knn + t_tab))
    if NPRED > 0:
        held = fit.info()["bytes"]
        a = fit.predict_knn_core(th, new, Xn, M)
        grid = fit.info()["bytes"] - held
        t0 = time.perf_counter()
        nnp = ca.vecchia_neighbours_pred(locs, new, M)
        t_tree = 1e3 * (time.perf_counter() - t0)
        nnp_dev = ca.vecchia_neighbours_pred_device(locs, new, M)
        b = fit.predict_core(th, new, Xn, nnp_dev)
        pr = max(reps // 2, 3)
        t_pk = timed(lambda: fit.predict_knn_core(th, new, Xn, M), pr)
        t_pc = timed(lambda: fit.predict_core(th, new, Xn, nnp), pr)
        t_pd = timed(lambda: ca.vecchia_neighbours_pred_device(locs, new, M), pr)
        say("  %7d predictions, predict_knn_core %10.3f ms (median %10.3f), chunks of %d rows; bits of predict_core with the "
            "exported table: %s" % ((NPRED,) + t_pk + (fit.info()["rows"], bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])))))
        say("    predict_core, table given      %10.3f ms (median %10.3f): the baseline, the path as it was before the search" % t_pc)
        say("    host.vecchia_neighbours_pred   %10.1f ms, once (the k-d tree query predict_core needs first): together %.1f ms, "
            "%.1f times predict_knn_core" % (t_tree, t_tree + t_pc[0], (t_tree + t_pc[0]) / t_pk[0]))
        say("    cocons_vecchia_neighbours, %d queries %10.3f ms (median %10.3f), stateless: grid built by every call" %
            ((NPRED,) + t_pd))
        say("  device bytes held: %.1f MB before the first predict_knn_core call, %.1f MB of grid added by it, %.1f MB after a second" %
            (held / 1e6, grid / 1e6, fit.info()["bytes"] / 1e6))
    fit.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
