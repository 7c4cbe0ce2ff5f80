"""Time the grouped Vecchia coefficient phase and the calls that start with it:
python tools/vecchia_group_coef_timing.py [n ...] [--m 30] [--max-rows 64] [--parent-lib FILE] [--limit SECONDS] [--out FILE].

For every n (default 10000 99856 1000000), in the setting of tools/vecchia_group_timing.py: uniform sites on the unit square in
random order, its design, wl.theta_full() -- the Bessel branch at a free smoothness --, one realisation, the m nearest earlier
neighbours found on the device, the greedy groups and their expanded table.  Every size runs in a child process of its own
under a time limit (--limit, default 420 seconds), so a size that hangs ends there and the sizes behind it are not started.
Timed after a warm-up with the host clock around calls that end in a device synchronise, the smallest of 20 calls (10 from
n = 10^6 on), the median and the largest:
  coefficient phase   the first of the three phases of cocons_debug_vecchia_sim_phases (ungrouped) and of
                      cocons_debug_vecchia_sim_phases_grouped on the same handle, by events on the handle's stream: the
                      records, the coefficient launch and the status word's way home;
  whole calls         unwhiten of 1 and of 16 columns, whiten_t of 1 column, leave-one-out and folds of 10, grouped against
                      ungrouped on the same handle, with "the same bits" per pair;
  the input table     the ungrouped calls on the handle of the INPUT table -- a coarser model, for orientation;
  the parent commit   with --parent-lib, the ungrouped entries by the library built from the parent commit, loaded beside this
                      one, on the expanded table: the same code, so the same bits and the same time within the spread.
Nothing is asserted; the lines also go to --out."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
LIMIT = int(_opt("--limit", 420))
OUT = _opt("--out", None)
CHILD = _opt("--child", None)
SIZES = [int(a) for a in sys.argv[1:]] or [10000, 99856, 1000000]


def say(text):
    print(text, flush=True)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts)), 1e3 * max(ts)


def phase(fit, entry, th, W, reps):
    """(smallest, median, largest) of the coefficient phase in device milliseconds"""
    from cocons_amd import host
    T = host.theta_table(th)
    out, ms3 = np.zeros(W.shape, order="F"), np.zeros(3)
    call = getattr(fit._L, entry)
    ts = []
    for k in range(reps + 1):
        rc = call(fit._h, host._p(T), int(W.shape[1]), host._p(W), host._p(out), host._p(ms3))
        assert rc == 0, (entry, rc)
        if k:
            ts.append(float(ms3[0]))
    return min(ts), float(np.median(ts)), max(ts)


class ParentLib:
    """the ungrouped entries of another build of the library"""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
        L.cocons_fit_create_vecchia.restype = ctypes.c_void_p
        L.cocons_fit_create_vecchia.argtypes = [ctypes.c_int] * 3 + [dp] * 4 + [ctypes.c_int, ctypes.c_int, ip]
        L.cocons_vecchia_unwhiten.restype = ctypes.c_int
        L.cocons_vecchia_unwhiten.argtypes = [ctypes.c_void_p, dp, ctypes.c_int, dp, dp]
        L.cocons_debug_vecchia_sim_phases.restype = ctypes.c_int
        L.cocons_debug_vecchia_sim_phases.argtypes = [ctypes.c_void_p, dp, ctypes.c_int, dp, dp, dp]
        L.cocons_vecchia_whiten_t.restype = ctypes.c_int
        L.cocons_vecchia_whiten_t.argtypes = [ctypes.c_void_p, dp, ctypes.c_int, dp, dp, dp]
        L.cocons_cv_vecchia.restype = ctypes.c_int
        L.cocons_cv_vecchia.argtypes = [ctypes.c_void_p, dp, dp, ctypes.c_int, ip, dp, dp, lp]
        L.cocons_fit_destroy.argtypes = [ctypes.c_void_p]
        self.L = L

    def handle(self, locs, X, z, nn):
        from cocons_amd import host, workloads as wl
        locs, X = host._f(locs), host._f(X)
        z = host._f(np.asarray(z, dtype=np.float64).reshape(X.shape[0], -1))
        nn = np.asfortranarray(nn, dtype=np.int32)
        lim = np.asarray(wl.SMOOTH_LIMITS, dtype=np.float64)
        h = self.L.cocons_fit_create_vecchia(X.shape[0], X.shape[1], z.shape[1], host._p(locs), host._p(X), host._p(z), host._p(lim),
                                             -1, nn.shape[1], host._ip(nn))
        assert h, "the parent library refused the handle"

        class Fit:
            _L, _h, n, r = self.L, h, X.shape[0], z.shape[1]

            def unwhiten_core(s, th, W):
                out = np.zeros(W.shape, order="F")
                assert s._L.cocons_vecchia_unwhiten(h, host._p(host.theta_table(th)), W.shape[1], host._p(W), host._p(out)) == 0
                return out

            def whiten_t_core(s, th, W):
                out, qd = np.zeros(W.shape, order="F"), np.zeros(s.n)
                assert s._L.cocons_vecchia_whiten_t(h, host._p(host.theta_table(th)), W.shape[1], host._p(W), host._p(out), host._p(qd)) == 0
                return out, qd

            def cv_core(s, th, fold=None):
                resid, var = np.zeros((s.n, s.r), order="F"), np.zeros(s.n)
                mean = np.ascontiguousarray(th["mean"], dtype=np.float64)
                nfold, lab = (0, None) if fold is None else host._fold_labels(fold, s.n)
                rc = s._L.cocons_cv_vecchia(h, host._p(host.theta_table(th)), host._p(mean), nfold, None if lab is None else host._ip(lab),
                                            host._p(resid), host._p(var), None)
                assert rc == 0, rc
                return resid, var

            def close(s):
                s._L.cocons_fit_destroy(h)

        return Fit()


def same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def calls(th, W1, W16, fold):
    """the whole calls that are timed: name -> (ungrouped form, grouped form), each taking the fit"""
    return (("unwhiten, 1 column", lambda f: f.unwhiten_core(th, W1), lambda f: f.unwhiten_grouped_core(th, W1)),
            ("unwhiten, 16 columns", lambda f: f.unwhiten_core(th, W16), lambda f: f.unwhiten_grouped_core(th, W16)),
            ("whiten_t, 1 column", lambda f: f.whiten_t_core(th, W1), lambda f: f.whiten_t_grouped_core(th, W1)),
            ("leave-one-out", lambda f: f.cv_core(th), lambda f: f.cv_core(th, grouped=True)),
            ("folds of 10", lambda f: f.cv_core(th, fold), lambda f: f.cv_core(th, fold, grouped=True)))


def one_size(n):
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    reps = 10 if n >= 1000000 else 20
    th = wl.theta_full()
    ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
    locs = np.random.default_rng(20260000 + n).uniform(0, 1, size=(n, 2))
    X, z = wl.design_from_locs(locs)["std.covs"], wl.synthetic_z(n)
    if "mean" not in th:
        th["mean"] = np.zeros(X.shape[1])
    nn = ca.vecchia_neighbours_device(locs, M)
    group, st = ca.vecchia_group(nn, CAP, stats=True)
    wide = ca.vecchia_group_table(nn, group)
    k = np.count_nonzero(wide, axis=1).astype(np.int64)
    pairs_b = int(np.sum(k * (k + 1) // 2))
    say("n = %d, m = %d, max_rows = %d, random order: %d blocks, %.2f rows and %.2f members per block on average, table width %d; "
        "pairs per observation %.1f (input table), %.1f (expanded table, ungrouped), %.1f (grouped)"
        % (n, M, CAP, st["blocks"], st["rows"] / st["blocks"], n / st["blocks"], wide.shape[1], st["pairs_ungrouped"] / n, pairs_b / n,
           st["pairs"] / n))
    rng = np.random.default_rng(5)
    W16 = np.asfortranarray(rng.standard_normal((n, 16)))
    W1 = np.asfortranarray(W16[:, :1])
    fold = rng.permutation(n) // 10
    fit = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, wide)
    fit.set_groups(group)
    pu = phase(fit, "cocons_debug_vecchia_sim_phases", th, W1, reps)
    pg = phase(fit, "cocons_debug_vecchia_sim_phases_grouped", th, W1, reps)
    say("  coefficient phase, expanded table: ungrouped %9.3f ms (median %9.3f, largest %9.3f)" % pu)
    say("  coefficient phase, expanded table: grouped   %9.3f ms (median %9.3f, largest %9.3f); grouped / ungrouped = %.3f in time "
        "against %.3f in pairs" % (pg + (pg[0] / pu[0], st["pairs"] / pairs_b)))
    table = calls(th, W1, W16, fold)
    times = {}
    for name, plain, grouped in table:
        tu, tg = timed(lambda: plain(fit), reps), timed(lambda: grouped(fit), reps)
        times[name] = tu
        say("  %-22s ungrouped %9.3f ms (median %9.3f, largest %9.3f)" % ((name + ":",) + tu))
        say("  %-22s grouped   %9.3f ms (median %9.3f, largest %9.3f); grouped / ungrouped = %.3f; the same bits: %s"
            % ((name + ":",) + tg + (tg[0] / tu[0], same(plain(fit), grouped(fit)))))
    want = {name: plain(fit) for name, plain, _ in table}
    fit.close()
    if PARENT:
        pf = ParentLib(PARENT).handle(locs, X, z, wide)
        pp = phase(pf, "cocons_debug_vecchia_sim_phases", th, W1, reps)
        say("  the parent commit's library, expanded table: coefficient phase %9.3f ms (median %9.3f, largest %9.3f); this "
            "library's / the parent's = %.3f" % (pp + (pu[0] / pp[0],)))
        for name, plain, _ in table:
            tp = timed(lambda: plain(pf), reps)
            say("  the parent commit's library, %-22s %9.3f ms (median %9.3f, largest %9.3f); this library's / the parent's = %.3f; "
                "the same bits: %s" % ((name + ":",) + tp + (times[name][0] / tp[0], same(plain(pf), want[name]))))
        pf.close()
    coarse = ca.CoconsVecchiaFit(locs, X, z, wl.SMOOTH_LIMITS, nn)
    pa = phase(coarse, "cocons_debug_vecchia_sim_phases", th, W1, reps)
    say("  the input table (a coarser model): coefficient phase %9.3f ms (median %9.3f, largest %9.3f)" % pa)
    for name, plain, _ in table:
        say("  the input table (a coarser model): %-22s %9.3f ms (median %9.3f, largest %9.3f)" % ((name + ":",) + timed(lambda: plain(coarse), reps)))
    coarse.close()


if CHILD is not None:
    one_size(int(CHILD))
    sys.exit(0)

lines = ["python tools/vecchia_group_coef_timing.py %s --m %d --max-rows %d%s" %
         (" ".join(map(str, SIZES)), M, CAP, " --parent-lib FILE" if PARENT else "")]
print(lines[0], flush=True)
status = 0
for n in SIZES:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--m", str(M), "--max-rows", str(CAP)]
    if PARENT:
        cmd += ["--parent-lib", PARENT]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LIMIT)
        text, status = res.stdout, res.returncode
    except subprocess.TimeoutExpired as e:
        text, status = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
        text += "n = %d: ended at the time limit of %d seconds\n" % (n, LIMIT)
    print(text, end="", flush=True)
    lines += text.splitlines()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if status:
        print("n = %d: exit status %d; the sizes behind it are not run" % (n, status), flush=True)
        break
sys.exit(status)
