"""Time the grouped Vecchia value call: python tools/vecchia_group_timing.py [n ...] [--m 30] [--max-rows 64]
[--parent-lib FILE] [--kl N] [--out FILE].

For every n (default 10000 99856 1000000), for uniform sites on the unit square in random order and in the maxmin order of
cocons_vecchia_order: the setting of tools/vecchia_timing.py (its design, wl.theta_full(), one realisation), the m nearest
earlier neighbours found on the device (cocons_vecchia_neighbours), the greedy groups of cocons_vecchia_group and their
expanded table.  Timed after a warm-up with the host clock around calls that end in a device synchronise, the smallest of 20
calls (and the median):
  (a) cocons_neg2loglik_vecchia on the INPUT table -- what a user pays today -- by this library and, with --parent-lib, by the
      library built from the parent commit, loaded beside this one;
  (b) cocons_neg2loglik_vecchia on the expanded table of the grouped handle (the same model as the grouped call);
  (g) cocons_neg2loglik_vecchia_grouped on that handle, the blocks dealt largest first and, on a second handle made under
      COCONS_VECCHIA_GROUP_ORDER=0, by block id.
Also: blocks, mean rows and mean members per block, pairs per observation of the three schedules, the host time of
cocons_vecchia_group and of cocons_vecchia_set_groups, the bytes the plan adds, and whether (g) returns the bits of (b).
--kl N (no GPU is used; nothing else is run): at tools/vecchia_order_kl.py's setting with N sites, the KL divergence of the
input-table model and of the grouped model from the exact one, in both orders.  Nothing is asserted; the lines also go to
--out."""
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
KL = int(_opt("--kl", 0))
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


def kl_report(n):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import knn_reference as KR
    import vecchia_reference as VR
    from oracle import oracle as O
    O.build()
    locs = np.random.default_rng(20260000 + n).uniform(0, 1, size=(n, 2))
    X = np.ones((n, 1), order="F")
    th = {"mean": np.zeros(1), "std.dev": np.zeros(1), "scale": np.array([np.log(0.15)]), "aniso": np.zeros(1), "tilt": np.zeros(1),
          "smooth": np.zeros(1), "nugget": np.array([np.log(1e-8)])}
    for name, o in (("random order", np.arange(n)), ("host.vecchia_order", host.vecchia_order(locs).astype(np.int64) - 1)):
        l = np.ascontiguousarray(locs[o])
        S = O.cov_rns(th, l, X, (0.5, 2.5))
        half_logdet = float(np.sum(np.log(np.diag(np.linalg.cholesky(S)))))
        nn = KR.brute_self(l, M)
        group, st = ca.vecchia_group(nn, CAP, stats=True)
        wide = ca.vecchia_group_table(nn, group)
        kl = [float(np.sum(VR.whiten(S, t, np.zeros((n, 1)))[1])) - half_logdet for t in (nn, wide)]
        say("n = %d, m = %d, max_rows = %d, %s: KL from the exact model %.3f on the input table, %.3f grouped (%d blocks, %.1f "
            "pairs per observation against %.1f)" % (n, M, CAP, name, kl[0], kl[1], st["blocks"], st["pairs"] / n,
                                                     st["pairs_ungrouped"] / n))


class ParentLib:
    """cocons_fit_create_vecchia, cocons_neg2loglik_vecchia and cocons_fit_destroy of another build of the library"""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        L.cocons_fit_create_vecchia.restype = ctypes.c_void_p
        L.cocons_fit_create_vecchia.argtypes = [ctypes.c_int] * 3 + [dp] * 4 + [ctypes.c_int, ctypes.c_int, ip]
        L.cocons_neg2loglik_vecchia.restype = ctypes.c_int
        L.cocons_neg2loglik_vecchia.argtypes = [ctypes.c_void_p, dp, dp, dp, dp]
        L.cocons_fit_destroy.argtypes = [ctypes.c_void_p]
        self.L = L

    def value_call(self, locs, X, z, nn, th):
        """(value, a closure that evaluates it again, a closure that frees the handle)"""
        locs, X = host._f(locs), host._f(X)
        z = host._f(np.asarray(z, dtype=np.float64).reshape(X.shape[0], -1))
        nn = np.asfortranarray(nn, dtype=np.int32)
        lim = np.asarray(wl.SMOOTH_LIMITS, dtype=np.float64)
        h = self.L.cocons_fit_create_vecchia(X.shape[0], X.shape[1], z.shape[1], host._p(locs), host._p(X), host._p(z), host._p(lim),
                                             -1, nn.shape[1], host._ip(nn))
        assert h, "the parent library refused the handle"
        T, mean = host._table_mean(th)
        val, parts = ctypes.c_double(0.0), np.zeros(1 + z.shape[1])

        def call():
            rc = self.L.cocons_neg2loglik_vecchia(h, host._p(T), host._p(mean), ctypes.byref(val), host._p(parts))
            assert rc == 0, rc
            return val.value

        return call(), call, lambda: self.L.cocons_fit_destroy(h)


def one_order(n, name, locs, th, parent):
    sc = wl.design_from_locs(locs)
    X, z = sc["std.covs"], wl.synthetic_z(n)
    nn = ca.vecchia_neighbours_device(locs, M)
    t0 = time.perf_counter()
    group, st = ca.vecchia_group(nn, CAP, stats=True)
    t_group = time.perf_counter() - t0
    wide = ca.vecchia_group_table(nn, group)
    members = np.bincount(group)
    say("n = %d, m = %d, max_rows = %d, %s: %d blocks, %.2f rows and %.2f members per block on average (largest %d members); "
        "expanded table of %d columns" % (n, M, CAP, name, st["blocks"], st["rows"] / st["blocks"], n / st["blocks"],
                                          int(members.max()), wide.shape[1]))
    pairs_b = int(np.sum(np.count_nonzero(wide, axis=1).astype(np.int64) * (np.count_nonzero(wide, axis=1) + 1) // 2))
    say("  pairs per observation: %.1f ungrouped on the input table (a), %.1f ungrouped on the expanded table (b), %.1f grouped (g)"
        % (st["pairs_ungrouped"] / n, pairs_b / n, st["pairs"] / n))
    say("  cocons_vecchia_group on the host: %.3f s" % t_group)
    plain = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    ta = timed(lambda: plain.neg2loglik_core(th))
    va = plain.neg2loglik_core(th)[0]
    plain.close()
    say("  (a) ungrouped value call, input table            %9.3f ms (median %9.3f); value %.6f" % (ta + (va,)))
    if parent:
        vp, call, free = parent.value_call(locs, X, z, nn, th)
        tp = timed(call)
        free()
        say("  (a) the same by the parent commit's library      %9.3f ms (median %9.3f); the same bits: %s" % (tp + (vp == va,)))
    fit = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    held = fit.info()["bytes"]
    t0 = time.perf_counter()
    info = fit.set_groups(group)
    t_set = time.perf_counter() - t0
    say("  cocons_vecchia_set_groups (table home, closure check, plan, upload): %.3f s; the plan adds %.2f MB to the handle's "
        "%.1f MB" % (t_set, (fit.info()["bytes"] - held) / 1e6, held / 1e6))
    tb = timed(lambda: fit.neg2loglik_core(th))
    tg = timed(lambda: fit.neg2loglik_core(th, grouped=True))
    vb, vg = fit.neg2loglik_core(th), fit.neg2loglik_core(th, grouped=True)
    fit.close()
    os.environ["COCONS_VECCHIA_GROUP_ORDER"] = "0"
    try:
        fit = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
        fit.set_groups(group)
    finally:
        del os.environ["COCONS_VECCHIA_GROUP_ORDER"]
    t0g = timed(lambda: fit.neg2loglik_core(th, grouped=True))
    v0 = fit.neg2loglik_core(th, grouped=True)
    fit.close()
    say("  (b) ungrouped value call, expanded table         %9.3f ms (median %9.3f); value %.6f" % (tb + (vb[0],)))
    say("  (g) grouped value call, blocks largest first     %9.3f ms (median %9.3f); the bits of (b): %s" %
        (tg + (vg[0] == vb[0] and np.array_equal(vg[1], vb[1]),)))
    say("  (g) grouped value call, blocks by id             %9.3f ms (median %9.3f); the bits of (b): %s" %
        (t0g + (v0[0] == vb[0] and np.array_equal(v0[1], vb[1]),)))
    say("  (g) / (b) = %.3f in time against %.3f in pairs; (g) / (a) = %.3f in time against %.3f in pairs" %
        (tg[0] / tb[0], info["pairs"] / pairs_b, tg[0] / ta[0], info["pairs"] / st["pairs_ungrouped"]))


say("python tools/vecchia_group_timing.py %s --m %d --max-rows %d%s" %
    (" ".join(map(str, SIZES)) if not KL else "--kl %d" % KL, M, CAP, " --parent-lib FILE" if PARENT else ""))
if KL:
    kl_report(KL)
    finish()
    sys.exit(0)
th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
parent = ParentLib(PARENT) if PARENT else None
for n in SIZES:
    locs = np.random.default_rng(20260000 + n).uniform(0, 1, size=(n, 2))
    one_order(n, "random order", locs, th, parent)
    order = ca.vecchia_order_device(locs).astype(np.int64) - 1
    one_order(n, "maxmin order", np.ascontiguousarray(locs[order]), th, parent)
    finish()
