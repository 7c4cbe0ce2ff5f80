"""Time the Vecchia entries on the device: python tools/vecchia_timing.py [n ...] [--m 30] [--pred 100000] [--fit N] [--out FILE].

For every n (default 10000 99856 1000000): uniform sites on the unit square in random order (the Vecchia order), the design
and theta of tools/taper_timing.py (wl.theta_full(), one realisation), the m nearest earlier neighbours from
host.vecchia_neighbours.  Timed after a warm-up, with the host clock around calls that end in a device synchronise (each
entry drains its stream before it returns): a value call, a value + gradient call (cocons_neg2loglik_grad_vecchia, set
against 2 P + 1 = 27 value calls: central differences over P = 13 parameters), a whiten of four columns, and `--pred`
predictions from their m nearest observations (0: none).  --fit N: at the size N, L-BFGS-B from a shifted start with
GetNeg2loglikelihoodVecchia_grad and with central differences of GetNeg2loglikelihoodVecchia, wall time and evaluations of
each.  Reported: the smallest and the median of the repetitions, the device bytes the handle holds
(cocons_vecchia_info) and the drop in free device memory across its creation.  Nothing is asserted; the lines also go to
--out."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca                     # noqa: E402
from cocons_amd import workloads as wl     # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


M = int(_opt("--m", 30))
NPRED = int(_opt("--pred", 100000))
FIT = int(_opt("--fit", 0))
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def device_free_bytes():
    from cocons_amd.shard import _hip_runtime
    hip = _hip_runtime()
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    return free.value


def timed(fn, reps):
    fn()                                     # warm-up: code objects, first allocations of the call's scratch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts))


th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_timing.py %s --m %d --pred %d" % (" ".join(map(str, SIZES)), M, NPRED))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    sc = wl.design_from_locs(locs)
    X, z = sc["std.covs"], wl.synthetic_z(n)
    new = rng.uniform(0, 1, size=(max(NPRED, 1), 2))
    Xn = wl.design_from_locs(new, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    t0 = time.perf_counter()
    nn = ca.vecchia_neighbours(locs, M)
    t_nn = time.perf_counter() - t0
    nnp = ca.vecchia_neighbours_pred(locs, new, M)
    B = np.asfortranarray(rng.standard_normal((n, 4)))
    free0 = device_free_bytes()
    t0 = time.perf_counter()
    fit = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    t_create = time.perf_counter() - t0
    reps = 20 if n <= 100000 else 10
    v = fit.neg2loglik_core(th)[0]
    tv = timed(lambda: fit.neg2loglik_core(th), reps)
    tw = timed(lambda: fit.whiten_core(th, B), reps)
    tp = timed(lambda: fit.predict_core(th, new, Xn, nnp), max(reps // 4, 3)) if NPRED > 0 else (0.0, 0.0)
    held = fit.info()["bytes"]
    g = fit.neg2loglik_grad_core(th)
    tg = timed(lambda: fit.neg2loglik_grad_core(th), reps)
    tv2 = timed(lambda: fit.neg2loglik_core(th), reps)
    info = fit.info()
    drop = free0 - device_free_bytes()
    say("n = %d, m = %d: neighbour search on the host %.1f s, handle created in %.2f s; value %.6f" % (n, M, t_nn, t_create, v))
    say("  value call            %9.3f ms (median %9.3f) over %d calls" % (tv + (reps,)))
    say("  value + gradient call %9.3f ms (median %9.3f); value bits kept: %s; 27 value calls: %.1f ms (value call again: %.3f ms)" %
        (tg + (g[0] == v, 27 * tv2[0], tv2[0])))
    say("  whiten, 4 columns     %9.3f ms (median %9.3f), host copies of n x 5 doubles included" % tw)
    say("  %7d predictions   %9.3f ms (median %9.3f), chunks of %d rows" % ((NPRED,) + tp + (info["rows"],)))
    say("  device bytes held: %.1f MB by the handle's own count, %.1f MB drop in free device memory" %
        (info["bytes"] / 1e6, drop / 1e6))
    say("  device bytes the first gradient call added: %.1f MB" % ((info["bytes"] - held) / 1e6))
    if n == FIT:
        from scipy.optimize import minimize
        pp = wl.par_pos_full()
        x0 = wl.theta_vector_from_lists(th, pp) + 0.05
        lam = (0.0, 0.0, 0.0)
        count = [0]

        def both(x):
            count[0] += 1
            return ca.GetNeg2loglikelihoodVecchia_grad(x, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)

        def value(x):
            count[0] += 1
            return ca.GetNeg2loglikelihoodVecchia(x, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)

        def central(x, h=1e-6):
            g = np.zeros_like(x)
            for i in range(x.size):
                e = np.zeros_like(x)
                e[i] = h
                g[i] = (value(x + e) - value(x - e)) / (2 * h)
            return g

        for name, kw in (("analytic gradient", dict(fun=both, jac=True)), ("central differences", dict(fun=value, jac=central))):
            count[0] = 0
            t0 = time.perf_counter()
            res = minimize(x0=x0, method="L-BFGS-B", options=dict(maxiter=200), **kw)
            say("  L-BFGS-B, P = %d, %s: %.2f s, %d iterations, %d evaluations, end value %.6f (%s)" %
                (x0.size, name, time.perf_counter() - t0, res.nit, count[0], res.fun, res.message))
    fit.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
