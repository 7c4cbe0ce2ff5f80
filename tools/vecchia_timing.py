"""Time the Vecchia entries on the device: python tools/vecchia_timing.py [n ...] [--m 30] [--pred 100000] [--fit N] [--fisher]
[--fisher-check N] [--out FILE].

For every n (default 10000 99856 1000000): uniform sites on the unit square in random order (the Vecchia order), the design
and theta of tools/taper_timing.py (wl.theta_full(), one realisation), the m nearest earlier neighbours from
host.vecchia_neighbours.  Timed after a warm-up, with the host clock around calls that end in a device synchronise (each
entry drains its stream before it returns): a value call, a value + gradient call (cocons_neg2loglik_grad_vecchia, set
against 2 P + 1 = 27 value calls: central differences over P = 13 parameters), a whiten of four columns, and `--pred`
predictions from their m nearest observations (0: none).  --fit N: at the size N, L-BFGS-B from a shifted start with
GetNeg2loglikelihoodVecchia_grad and with central differences of GetNeg2loglikelihoodVecchia, wall time and evaluations of
each.  --fisher: one cocons_fisher_vecchia call with the P = 16 rows of the optimiser's Jacobian as directions, beside the
value + gradient call and 2 P of them (the differencing route to an observed Hessian), and the bytes its first call added;
--fisher-check N: at the size N, sqrt(diag(inv(.))) of getFisher_vecchia against the same of central differences of
GetNeg2loglikelihoodVecchia_grad (half the value's Hessian) at theta, for data drawn from the Vecchia model at theta, the
largest relative gap and the step.  Reported: the smallest and the median of the repetitions, the device bytes the handle holds
(cocons_vecchia_info) and the drop in free device memory across its creation.  Nothing is asserted; the lines also go to
--out."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca                     # noqa: E402
from cocons_amd import host, workloads as wl     # noqa: E402


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
FISHER_CHECK = int(_opt("--fisher-check", 0))
FISHER = "--fisher" in sys.argv
if FISHER:
    sys.argv.remove("--fisher")
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


def vecchia_draw(th, locs, X, nn, rng):
    """z ~ the Vecchia model at th with zero mean: z_i = c' K^-1 z[nb] + sqrt(C_ii - c' K^-1 c) e_i, row after row"""
    from oracle import oracle as O
    O.build()
    n = X.shape[0]
    z, e = np.zeros(n), rng.standard_normal(n)
    for i in range(n):
        nb = np.sort(nn[i][nn[i] > 0]) - 1
        idx = np.append(nb, i)
        L = np.linalg.cholesky(O.cov_rns(th, locs[idx], X[idx], wl.SMOOTH_LIMITS))
        z[i] = L[-1, :-1] @ np.linalg.solve(L[:-1, :-1], z[nb]) + L[-1, -1] * e[i] if nb.size else L[-1, -1] * e[i]
    return z


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
say("python tools/vecchia_timing.py %s --m %d --pred %d%s%s" % (" ".join(map(str, SIZES)), M, NPRED, " --fisher" if FISHER else "",
                                                            " --fisher-check %d" % FISHER_CHECK if FISHER_CHECK else ""))
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
    if FISHER:
        pp = wl.par_pos_full()
        par = wl.theta_vector_from_lists(th, pp)
        Jt, _ = host.fisher_jacobian(par, pp)
        held = fit.info()["bytes"]
        fi = fit.fisher_core(th, Jt)
        tf = timed(lambda: fit.fisher_core(th, Jt), reps)
        tg2 = timed(lambda: fit.neg2loglik_grad_core(th), reps)
        say("  information call, %2d directions %9.3f ms (median %9.3f); value + gradient call again: %.3f ms (%.2f of them); "
            "%d gradient calls: %.1f ms" % ((Jt.shape[0],) + tf + (tg2[0], tf[0] / tg2[0], 2 * par.size, 2 * par.size * tg2[0])))
        say("  device bytes the first information call added: %.1f MB; symmetric to the bit: %s" %
            ((fit.info()["bytes"] - held) / 1e6, np.array_equal(fi[0], fi[0].T)))
        if n == FISHER_CHECK:
            # data drawn from the Vecchia model at theta itself (row by row on the host, the blocks from the CPU oracle), so that
            # the observed Hessian at theta differs from the expected information by a term of zero mean
            zs = vecchia_draw(th, locs, X, nn, np.random.default_rng(7))
            fs = ca.CoconsVecchiaFit(locs, X, zs, wl.SMOOTH_LIMITS, nn)
            lam, h = (0.0, 0.0, 0.0), 1e-4

            def grad(x):
                return ca.GetNeg2loglikelihoodVecchia_grad(x, pp, nn, locs, X, wl.SMOOTH_LIMITS, zs, n, lam, fit=fs)[1]

            info = ca.getFisher_vecchia(par, pp, locs, X, wl.SMOOTH_LIMITS, zs, n, nn, fit=fs)
            H = np.zeros((par.size, par.size))
            for i in range(par.size):
                e = np.zeros_like(par)
                e[i] = h
                H[i] = (grad(par + e) - grad(par - e)) / (4 * h)          # half the value: the negative log-likelihood
            fs.close()
            with np.errstate(invalid="ignore"):
                se_i, se_h = np.sqrt(np.diag(np.linalg.inv(info))), np.sqrt(np.diag(np.linalg.inv(0.5 * (H + H.T))))
            say("  standard errors at theta for data drawn from the Vecchia model at theta, expected information against central "
                "differences of the gradient (step %g): largest relative gap %.3g; asymmetry of the differenced Hessian %.2e of its "
                "largest entry" % (h, float(np.max(np.abs(se_i - se_h) / se_h)), float(np.max(np.abs(H - H.T)) / np.max(np.abs(H)))))
            say("    expected: " + " ".join("%.3g" % v for v in se_i))
            say("    observed: " + " ".join("%.3g" % v for v in se_h))
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
