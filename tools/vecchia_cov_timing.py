"""Time U^-T on a Vecchia fit: python tools/vecchia_cov_timing.py [n ...] [--m 30] [--sorted-up-to 100000] [--star 1000000]
[--tiers 1] [--out FILE].

The setting of tools/vecchia_cv_timing.py: for every n (default 10000 99856 1000000) uniform sites on the unit square in random
order, in the maxmin order (CoconsVecchiaFit.from_maxmin) and, for n up to --sorted-up-to, sorted by x (an adversarial order: a
deep dependency graph, tools/vecchia_sim_timing.py's), the design and theta of tools/taper_timing.py, the m nearest
earlier rows found on the device.  Timed with the host clock around calls that end in a device synchronise, the smallest and the
median of several calls after a warm-up, the two settings of COCONS_VECCHIA_SOLVE_T_FUSE in alternation (the library reads the
switch at every call), and by events on the handle's stream (cocons_debug_vecchia_solve_t_phases):
  - the transposed schedule of a fresh handle (its first call): depth, widest level, longest list, rows of the wide tier, launches
    of one solve with and without fused runs, device bytes, and the milliseconds of building it;
  - cocons_vecchia_unwhiten_t, cocons_vecchia_cov_mult and cocons_vecchia_cov_cols with 1 and 16 columns, host copies included,
    and whether the two settings of the switch give the same bits;
  - the comparators, on the same handle in the same visit: cocons_vecchia_unwhiten (U^-1 moves the same n m coefficients) and
    cocons_vecchia_whiten_t (U' reads the same lists), with the ratio of cocons_vecchia_unwhiten_t to each;
  - the earlier entries once, ungrouped and (n <= 10000) grouped, as a record that they run as before;
  - --star: the star table (every row names row 1) of that many rows: one list of n - 1 rows in the workgroup tier, and the same
    list summed by one wavefront (COCONS_VECCHIA_SOLVE_T_WIDE moved out of reach);
  - --tiers: star tables whose one list has 128 .. 65536 rows, the solve's launches by events with the list in the workgroup tier
    and in the one-wave tier: what VECCHIA_SOLVE_T_WIDE is chosen from.
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
STAR = int(_opt("--star", 1000000))
TIERS = int(_opt("--tiers", 1))
OUT = _opt("--out", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]
SWITCH, WIDE = "COCONS_VECCHIA_SOLVE_T_FUSE", "COCONS_VECCHIA_SOLVE_T_WIDE"
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
    """(ms coefficients, ms transposed schedule, ms transposed solve) of one cocons_vecchia_unwhiten_t, by events"""
    T = host.theta_table(th)
    out, ms = np.zeros(W.shape, order="F"), np.zeros(3)
    _lib.check(fit._L.cocons_debug_vecchia_solve_t_phases(fit._h, host._p(T), 0, int(W.shape[1]), host._p(W), host._p(out),
                                                          host._p(ms)), "cocons_debug_vecchia_solve_t_phases")
    return ms


def tiers():
    import ctypes
    out = (ctypes.c_int * 4)()
    _lib.load().cocons_debug_vecchia_solve_t_tiers(out)
    return [int(v) for v in out]


def star_fit(n):
    locs = np.random.default_rng(7).uniform(0, 1, size=(n, 2))
    nn = np.ones((n, 1), dtype=np.int32, order="F")
    nn[0, 0] = 0
    return ca.CoconsVecchiaFit(locs, np.asfortranarray(np.column_stack([np.ones(n), locs])), np.zeros(n), wl.SMOOTH_LIMITS, nn)


th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
say("python tools/vecchia_cov_timing.py %s --m %d --sorted-up-to %d --star %d --tiers %d" %
    (" ".join(map(str, SIZES)), M, SORTED_UP_TO, STAR, TIERS))
say("tiers: a list of more than %d rows is summed by a workgroup of %d threads; %d columns a group; a fused level has at most %d "
    "items" % tuple(tiers()))
for n in SIZES:
    rng = np.random.default_rng(20260000 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    X, z = wl.design_from_locs(locs)["std.covs"], wl.synthetic_z(n)
    W = np.asfortranarray(np.random.default_rng(n + 1).standard_normal((n, 16)))
    W1 = np.asfortranarray(W[:, :1])
    reps = 10 if n <= 100000 else 4
    for order in ("random", "maxmin", "sorted by x"):
        if order == "sorted by x" and n > SORTED_UP_TO:
            continue
        make = ca.CoconsVecchiaFit.from_maxmin if order == "maxmin" else ca.CoconsVecchiaFit.from_knn
        by_x = np.argsort(locs[:, 0], kind="stable")
        fit = make(locs[by_x], np.asfortranarray(X[by_x]), z, wl.SMOOTH_LIMITS, M) if order == "sorted by x" else \
            make(locs, X, z, wl.SMOOTH_LIMITS, M)
        fuse(True)
        longest = fit.transpose()["longest"]                # the lists are made here, not in the timed first call
        t0 = time.perf_counter()
        first = phases(fit, th, W1)                         # the handle's first call: the transposed schedule is made in it
        t_first = 1e3 * (time.perf_counter() - t0)
        s_on = fit.schedule_t()
        fuse(False)
        s_off = fit.schedule_t()
        fuse(True)
        fwd = fit.schedule()
        sizes = np.bincount(s_on["levels"])[1:]
        lens = np.diff(fit.transpose()["ptr"])
        say("n = %d, m = %d, %s order: transposed depth %d (forward %d), widest level %d rows, median level %d rows, longest list "
            "%d, %d rows in the workgroup tier; launches of one solve %d with fused runs, %d without; transposed schedule %.1f MB "
            "on the device" % (n, M, order, s_on["depth"], fwd["depth"], s_on["widest"], int(np.median(sizes)), longest,
                               int(np.sum(lens > tiers()[0])), s_on["launches"], s_off["launches"], s_on["bytes"] / 1e6))
        say("  first call of the handle (c = 1) %10.3f ms by the host clock; by events: coefficients %.3f ms, transposed schedule "
            "%.3f ms, transposed solve %.3f ms" % (t_first, first[0], first[1], first[2]))
        idx1, idx16 = np.array([n]), np.linspace(1, n, 16).astype(np.int64)
        base = {}
        for name, fn in (("cocons_vecchia_unwhiten", fit.unwhiten_core), ("cocons_vecchia_whiten_t", fit.whiten_t_core)):
            for c, Wc in ((1, W1), (16, W)):
                base[name, c] = timed(lambda: fn(th, Wc), reps)
                say("  %-26s c = %-2d %10.3f ms (median %10.3f) over %d calls, host copies included: the comparator" %
                    ((name, c) + base[name, c] + (reps,)))
        for name, fn, args in (("cocons_vecchia_unwhiten_t", fit.unwhiten_t_core, {1: W1, 16: W}),
                               ("cocons_vecchia_cov_mult", fit.cov_mult_core, {1: W1, 16: W}),
                               ("cocons_vecchia_cov_cols", fit.cov_cols_core, {1: idx1, 16: idx16})):
            for c in (1, 16):
                (on, off) = timed_pair(lambda: fn(th, args[c]), reps)
                fuse(True)
                a = fn(th, args[c])
                fuse(False)
                b = fn(th, args[c])
                fuse(True)
                say("  %-26s c = %-2d fused runs %10.3f ms (median %10.3f), one launch per level and tier %10.3f ms (median "
                    "%10.3f) over %d calls each, alternating, host copies included; same bits: %s" %
                    ((name, c) + on + off + (reps, bool(np.array_equal(a, b)))))
                if name == "cocons_vecchia_unwhiten_t":
                    say("    %.2f of cocons_vecchia_unwhiten, %.2f of cocons_vecchia_whiten_t at the same c (the smallest times)" %
                        (on[0] / base["cocons_vecchia_unwhiten", c][0], on[0] / base["cocons_vecchia_whiten_t", c][0]))
                    p_on = min((phases(fit, th, args[c]) for _ in range(reps)), key=lambda v: v.sum())
                    fuse(False)
                    p_off = min((phases(fit, th, args[c]) for _ in range(reps)), key=lambda v: v.sum())
                    fuse(True)
                    say("    by events (the call of %d with the smallest sum): coefficients %.3f ms, transposed solve %.3f ms with "
                        "fused runs; coefficients %.3f ms, transposed solve %.3f ms with one launch per level and tier" %
                        (reps, p_on[0], p_on[2], p_off[0], p_off[2]))
        t_val = timed(lambda: fit.neg2loglik_core(th), reps)
        say("  cocons_neg2loglik_vecchia        %10.3f ms (median %10.3f): the yardstick of the coefficient phase" % t_val)
        fit.close()
    if n <= 10000:
        g = ca.CoconsVecchiaFit.from_groups_knn(locs, X, z, wl.SMOOTH_LIMITS, M)
        for name, plain, grouped in (("unwhiten", g.unwhiten_core, g.unwhiten_grouped_core),
                                     ("whiten_t", lambda t, w: g.whiten_t_core(t, w)[0], lambda t, w: g.whiten_t_grouped_core(t, w)[0]),
                                     ("unwhiten_t", g.unwhiten_t_core, lambda t, w: g.unwhiten_t_core(t, w, grouped=True)),
                                     ("cov_mult", g.cov_mult_core, lambda t, w: g.cov_mult_core(t, w, grouped=True))):
            tp, tg = timed(lambda: plain(th, W), reps), timed(lambda: grouped(th, W), reps)
            say("  grouped handle (expanded table), %-10s c = 16: per row %10.3f ms, per block %10.3f ms; same bits: %s" %
                (name, tp[0], tg[0], bool(np.array_equal(plain(th, W), grouped(th, W)))))
        g.close()
if STAR > 0:
    n = STAR
    W = np.asfortranarray(np.random.default_rng(n + 1).standard_normal((n, 16)))
    for wide in (None, str(2 ** 31 - 1)):
        if wide is None:
            os.environ.pop(WIDE, None)
        else:
            os.environ[WIDE] = wide
        fit = star_fit(n)
        fit.transpose()
        first = phases(fit, th, W[:, :1])
        s = fit.schedule_t()
        say("star table, n = %d (one list of %d rows), the list in the %s tier: depth %d, launches %d; first call by events: "
            "coefficients %.3f ms, transposed schedule %.3f ms, transposed solve %.3f ms" %
            (n, n - 1, "workgroup" if wide is None else "one-wave", s["depth"], s["launches"], first[0], first[1], first[2]))
        for c in (1, 16):
            p = min((phases(fit, th, W[:, :c]) for _ in range(5)), key=lambda v: v[2])
            t = timed(lambda: fit.unwhiten_t_core(th, W[:, :c]), 4)
            tc = timed(lambda: fit.cov_mult_core(th, W[:, :c]), 4)
            tu = timed(lambda: fit.unwhiten_core(th, W[:, :c]), 4)
            tw = timed(lambda: fit.whiten_t_core(th, W[:, :c]), 4)
            say("  c = %-2d transposed solve %.3f ms by events (coefficients %.3f ms); unwhiten_t %.3f ms, cov_mult %.3f ms, "
                "unwhiten %.3f ms, whiten_t %.3f ms by the host clock, host copies included" %
                (c, p[2], p[0], t[0], tc[0], tu[0], tw[0]))
        fit.close()
    os.environ.pop(WIDE, None)
if TIERS:
    say("the tiers: star tables of L + 1 rows, the transposed solve's launches by events, the smallest of 20 calls, the one list of "
        "L rows in the workgroup tier / in the one-wave tier")
    for L in (128, 256, 512, 1024, 2048, 4096, 16384, 65536):
        n = L + 1
        W = np.asfortranarray(np.random.default_rng(n + 1).standard_normal((n, 16)))
        row = []
        for wide in ("0", str(2 ** 31 - 1)):
            os.environ[WIDE] = wide
            fit = star_fit(n)
            phases(fit, th, W[:, :1])
            row += [min(phases(fit, th, W[:, :c])[2] for _ in range(20)) for c in (1, 16)]
            fit.close()
        say("  L = %-6d c = 1: workgroup %.4f ms, one wave %.4f ms; c = 16: workgroup %.4f ms, one wave %.4f ms" %
            (L, row[0], row[2], row[1], row[3]))
    os.environ.pop(WIDE, None)
os.environ.pop(SWITCH, None)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
