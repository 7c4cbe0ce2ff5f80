"""Time the grouped Vecchia gradient call: python tools/vecchia_group_grad_timing.py [n ...] [--m 30]
[--max-rows 64] [--parent-lib FILE] [--fit N] [--out FILE].

For every n (default 10000 99856 1000000), for uniform sites on the unit square in random order and in the maxmin order of
cocons_vecchia_order: the setting of tools/vecchia_group_timing.py (its design, wl.theta_full() -- the Bessel branch at a free
smoothness --, one realisation, the m nearest earlier neighbours found on the device, the greedy groups and their expanded
table).  Timed after a warm-up with the host clock around calls that end in a device synchronise, the smallest of 20 calls
(and the median):
  (g) cocons_neg2loglik_grad_vecchia_grouped on the grouped handle;
  (b) cocons_neg2loglik_grad_vecchia on the same handle -- the same model, the figure (g) is judged against -- by this library
      and, with --parent-lib, by the library built from the parent commit, loaded beside this one;
  (a) cocons_neg2loglik_grad_vecchia on the INPUT table -- a coarser model;
  (v) cocons_neg2loglik_vecchia_grouped, the grouped value call.
Also the pairs per observation of the three schedules and the largest relative deviation of (g)'s gradient from (b)'s.  --fit N: at the size N, L-BFGS-B from a shifted start (tools/vecchia_timing.py's run)
with the grouped gradient and with the ungrouped gradient on the same handle: times, evaluation counts and end values.
Nothing is asserted; the lines also go to --out."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
CAP = int(_opt("--max-rows", 64))
PARENT = _opt("--parent-lib", None)
FIT = int(_opt("--fit", 0))
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
LINES = []
REPS = 20


def say(text):
    print(text, flush=True)
    LINES.append(text)


def finish():
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts))


class ParentLib:
    """cocons_fit_create_vecchia, cocons_neg2loglik_grad_vecchia and cocons_fit_destroy of another build of the library"""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        L.cocons_fit_create_vecchia.restype = ctypes.c_void_p
        L.cocons_fit_create_vecchia.argtypes = [ctypes.c_int] * 3 + [dp] * 4 + [ctypes.c_int, ctypes.c_int, ip]
        L.cocons_neg2loglik_grad_vecchia.restype = ctypes.c_int
        L.cocons_neg2loglik_grad_vecchia.argtypes = [ctypes.c_void_p, dp, dp, ctypes.c_int] + [dp] * 6
        L.cocons_fit_destroy.argtypes = [ctypes.c_void_p]
        self.L = L

    def grad_call(self, locs, X, z, nn, th):
        """(gradient table, a closure that evaluates it again, a closure that frees the handle)"""
        locs, X = host._f(locs), host._f(X)
        z = host._f(np.asarray(z, dtype=np.float64).reshape(X.shape[0], -1))
        nn = np.asfortranarray(nn, dtype=np.int32)
        lim = np.asarray(wl.SMOOTH_LIMITS, dtype=np.float64)
        p = X.shape[1]
        h = self.L.cocons_fit_create_vecchia(X.shape[0], p, z.shape[1], host._p(locs), host._p(X), host._p(z), host._p(lim),
                                             -1, nn.shape[1], host._ip(nn))
        assert h, "the parent library refused the handle"
        T, mean = host._table_mean(th)
        val, parts = np.zeros(1), np.zeros(1 + z.shape[1])
        gt, gq, gm = np.zeros((6, p)), np.zeros((6, p)), np.zeros(p)

        def call():
            rc = self.L.cocons_neg2loglik_grad_vecchia(h, host._p(T), host._p(mean), 0, None, host._p(val), host._p(parts),
                                                       host._p(gt), host._p(gq), host._p(gm))
            assert rc == 0, rc
            return gt

        return call().copy(), call, lambda: self.L.cocons_fit_destroy(h)


def one_order(n, name, locs, th, parent):
    sc = wl.design_from_locs(locs)
    X, z = sc["std.covs"], wl.synthetic_z(n)
    nn = ca.vecchia_neighbours_device(locs, M)
    group, st = ca.vecchia_group(nn, CAP, stats=True)
    wide = ca.vecchia_group_table(nn, group)
    k = np.count_nonzero(wide, axis=1).astype(np.int64)
    pairs_b = int(np.sum(k * (k + 1) // 2))
    say("n = %d, m = %d, max_rows = %d, %s: %d blocks, %.2f rows and %.2f members per block on average; pairs per observation "
        "%.1f (a), %.1f (b), %.1f (g)" % (n, M, CAP, name, st["blocks"], st["rows"] / st["blocks"], n / st["blocks"],
                                          st["pairs_ungrouped"] / n, pairs_b / n, st["pairs"] / n))
    plain = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    ta = timed(lambda: plain.neg2loglik_grad_core(th))
    plain.close()
    fit = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    fit.set_groups(group)
    tb = timed(lambda: fit.neg2loglik_grad_core(th))
    tg = timed(lambda: fit.neg2loglik_grad_core(th, grouped=True))
    tv = timed(lambda: fit.neg2loglik_core(th, grouped=True))
    b, g = fit.neg2loglik_grad_core(th), fit.neg2loglik_grad_core(th, grouped=True)
    fits = []
    if n == FIT:
        from scipy.optimize import minimize
        pp = wl.par_pos_full()
        x0 = wl.theta_vector_from_lists(th, pp) + 0.05
        for grouped in (True, False):
            count = [0]

            def both(x):
                count[0] += 1
                return ca.GetNeg2loglikelihoodVecchia_grad(x, pp, nn, locs, X, wl.SMOOTH_LIMITS, z, n, (0.0, 0.0, 0.0), fit=fit,
                                                           grouped=grouped)

            t0 = time.perf_counter()
            res = minimize(fun=both, jac=True, x0=x0, method="L-BFGS-B", options=dict(maxiter=200))
            fits.append("  L-BFGS-B, P = %d, %s gradient on the grouped handle: %.2f s, %d iterations, %d evaluations, end value %.6f (%s)"
                        % (x0.size, "grouped" if grouped else "ungrouped", time.perf_counter() - t0, res.nit, count[0], res.fun, res.message))
    fit.close()
    dev = max(float(np.max(np.abs(g[i] - b[i])) / np.max(np.abs(b[2]))) for i in (2, 3))
    dev = max(dev, float(np.max(np.abs(g[4] - b[4])) / np.max(np.abs(b[4]))))
    say("  (g) grouped gradient call                        %9.3f ms (median %9.3f); value and parts the bits of (b): %s; "
        "gradient within %.1e of (b)" % (tg + (g[0] == b[0] and np.array_equal(g[1], b[1]), dev)))
    say("  (b) ungrouped gradient call, expanded table      %9.3f ms (median %9.3f)" % tb)
    if parent:
        gp, call, free = parent.grad_call(locs, X, z, wide, th)
        tp = timed(call)
        free()
        say("  (b) the same by the parent commit's library      %9.3f ms (median %9.3f); the same bits: %s" %
            (tp + (np.array_equal(gp, b[2]),)))
    say("  (a) ungrouped gradient call, input table         %9.3f ms (median %9.3f)" % ta)
    say("  (v) grouped value call                           %9.3f ms (median %9.3f)" % tv)
    say("  (g) / (b) = %.3f in time against %.3f in pairs; (g) / (a) = %.3f in time against %.3f in pairs; (g) / (v) = %.2f" %
        (tg[0] / tb[0], st["pairs"] / pairs_b, tg[0] / ta[0], st["pairs"] / st["pairs_ungrouped"], tg[0] / tv[0]))
    for line in fits:
        say(line)


say("python tools/vecchia_group_grad_timing.py %s --m %d --max-rows %d%s%s" %
    (" ".join(map(str, SIZES)), M, CAP, " --parent-lib FILE" if PARENT else "", " --fit %d" % FIT if FIT else ""))
th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
parent = ParentLib(PARENT) if PARENT else None
for n in SIZES:
    locs = np.random.default_rng(20260000 + n).uniform(0, 1, size=(n, 2))
    one_order(n, "random order", locs, th, parent)
    order = ca.vecchia_order_device(locs).astype(np.int64) - 1
    one_order(n, "maxmin order", np.ascontiguousarray(locs[order]), th, parent)
    finish()
