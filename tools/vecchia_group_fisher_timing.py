"""Time the grouped Vecchia information call: python tools/vecchia_group_fisher_timing.py [n ...] [--m 30]
[--max-rows 64] [--parent-lib FILE] [--out FILE].

For every n (default 10000 99856 1000000), for uniform sites on the unit square in random order and in the maxmin order of
cocons_vecchia_order: the setting of tools/vecchia_group_timing.py (its design, wl.theta_full() -- the Bessel branch at a free
smoothness --, one realisation, the m nearest earlier neighbours found on the device, the greedy groups and their expanded
table), with the P = 16 rows of the optimiser's Jacobian as directions.  Timed after a warm-up with the host clock around
calls that end in a device synchronise, the smallest of 20 calls (10 from n = 10^6 on) and the median:
  (g)  cocons_fisher_vecchia_grouped on the grouped handle;
  (b)  cocons_fisher_vecchia on the same handle -- the same model, the figure (g) is judged against -- by this library and,
       with --parent-lib, by the library built from the parent commit, loaded beside this one;
  (a)  cocons_fisher_vecchia on the INPUT table -- a coarser model;
  (gg) cocons_neg2loglik_grad_vecchia_grouped, the grouped gradient call.
Also the pairs per observation of the three schedules and the distance of (g) from (b) in fisher_reference's metric
(max |I_ab - R_ab| / sqrt(R_aa R_bb)).  Nothing is asserted; the lines also go to --out."""
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
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def finish():
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
    return 1e3 * min(ts), 1e3 * float(np.median(ts)), 1e3 * max(ts)


def metric(I, R):
    d = np.sqrt(np.where(np.diag(R) == 0, 1.0, np.diag(R)))
    return float(np.max(np.abs(np.asarray(I) - R) / np.outer(d, d)))


class ParentLib:
    """cocons_fit_create_vecchia, cocons_fisher_vecchia and cocons_fit_destroy of another build of the library"""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        L.cocons_fit_create_vecchia.restype = ctypes.c_void_p
        L.cocons_fit_create_vecchia.argtypes = [ctypes.c_int] * 3 + [dp] * 4 + [ctypes.c_int, ctypes.c_int, ip]
        L.cocons_fisher_vecchia.restype = ctypes.c_int
        L.cocons_fisher_vecchia.argtypes = [ctypes.c_void_p, dp, ctypes.c_int, dp, dp, dp]
        L.cocons_fit_destroy.argtypes = [ctypes.c_void_p]
        self.L = L

    def fisher_call(self, locs, X, z, nn, th, D):
        """(info, a closure that evaluates it again, a closure that frees the handle)"""
        locs, X = host._f(locs), host._f(X)
        z = host._f(np.asarray(z, dtype=np.float64).reshape(X.shape[0], -1))
        nn = np.asfortranarray(nn, dtype=np.int32)
        lim = np.asarray(wl.SMOOTH_LIMITS, dtype=np.float64)
        p = X.shape[1]
        h = self.L.cocons_fit_create_vecchia(X.shape[0], p, z.shape[1], host._p(locs), host._p(X), host._p(z), host._p(lim),
                                             -1, nn.shape[1], host._ip(nn))
        assert h, "the parent library refused the handle"
        T = host.theta_table(th)
        D = np.ascontiguousarray(np.asarray(D, dtype=np.float64).reshape(-1, 6 * p))
        info, im = np.zeros((D.shape[0], D.shape[0])), np.zeros((p, p))

        def call():
            rc = self.L.cocons_fisher_vecchia(h, host._p(T), D.shape[0], host._p(D), host._p(info), host._p(im))
            assert rc == 0, rc
            return info

        return call().copy(), call, lambda: self.L.cocons_fit_destroy(h)


def one_order(n, name, locs, th, Jt, parent):
    reps = 10 if n >= 1000000 else 20
    sc = wl.design_from_locs(locs)
    X, z = sc["std.covs"], wl.synthetic_z(n)
    nn = ca.vecchia_neighbours_device(locs, M)
    group, st = ca.vecchia_group(nn, CAP, stats=True)
    wide = ca.vecchia_group_table(nn, group)
    k = np.count_nonzero(wide, axis=1).astype(np.int64)
    pairs_b = int(np.sum(k * (k + 1) // 2))
    say("n = %d, m = %d, max_rows = %d, %s, %d directions: %d blocks, %.2f rows and %.2f members per block on average; pairs per "
        "observation %.1f (a), %.1f (b), %.1f (g)" % (n, M, CAP, name, Jt.shape[0], st["blocks"], st["rows"] / st["blocks"],
                                                      n / st["blocks"], st["pairs_ungrouped"] / n, pairs_b / n, st["pairs"] / n))
    plain = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    ta = timed(lambda: plain.fisher_core(th, Jt), reps)
    plain.close()
    fit = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    fit.set_groups(group)
    tb = timed(lambda: fit.fisher_core(th, Jt), reps)
    tg = timed(lambda: fit.fisher_core(th, Jt, grouped=True), reps)
    tgg = timed(lambda: fit.neg2loglik_grad_core(th, grouped=True), reps)
    b, g = fit.fisher_core(th, Jt), fit.fisher_core(th, Jt, grouped=True)
    fit.close()
    say("  (g)  grouped information call                     %9.3f ms (median %9.3f, largest %9.3f); within %.1e of (b) in the "
        "metric, info_mean within %.1e" % (tg + (metric(g[0], b[0]), float(np.max(np.abs(g[1] - b[1])) / np.max(np.abs(b[1]))))))
    say("  (b)  ungrouped information call, expanded table   %9.3f ms (median %9.3f, largest %9.3f)" % tb)
    if parent:
        ip, call, free = parent.fisher_call(locs, X, z, wide, th, Jt)
        tp = timed(call, reps)
        free()
        say("  (b)  the same by the parent commit's library      %9.3f ms (median %9.3f, largest %9.3f); the same bits: %s" %
            (tp + (np.array_equal(ip, b[0]),)))
    say("  (a)  ungrouped information call, input table      %9.3f ms (median %9.3f, largest %9.3f)" % ta)
    say("  (gg) grouped gradient call                        %9.3f ms (median %9.3f, largest %9.3f)" % tgg)
    say("  (g) / (b) = %.3f in time against %.3f in pairs; (g) / (a) = %.3f in time against %.3f in pairs; (g) / (gg) = %.2f" %
        (tg[0] / tb[0], st["pairs"] / pairs_b, tg[0] / ta[0], st["pairs"] / st["pairs_ungrouped"], tg[0] / tgg[0]))


say("python tools/vecchia_group_fisher_timing.py %s --m %d --max-rows %d%s" %
    (" ".join(map(str, SIZES)), M, CAP, " --parent-lib FILE" if PARENT else ""))
th = wl.theta_full()
pp = wl.par_pos_full()
Jt, _ = host.fisher_jacobian(wl.theta_vector_from_lists(th, pp), pp)
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
parent = ParentLib(PARENT) if PARENT else None
for n in SIZES:
    locs = np.random.default_rng(20260000 + n).uniform(0, 1, size=(n, 2))
    one_order(n, "random order", locs, th, Jt, parent)
    order = ca.vecchia_order_device(locs).astype(np.int64) - 1
    one_order(n, "maxmin order", np.ascontiguousarray(locs[order]), th, Jt, parent)
    finish()
