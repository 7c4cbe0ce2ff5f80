"""Time the grouping of Vecchia rows on the device: python tools/vecchia_group_device_timing.py [n ...] [--m 30]
[--max-rows 64] [--parent-lib FILE] [--out FILE].

For every n (default 10000 99856 1000000), for uniform sites on the unit square in random order and in the maxmin order of
cocons_vecchia_order, tools/vecchia_group_timing.py's setting (its design, wl.theta_full(), one realisation) and the m nearest
earlier neighbours found on the device.  Timed with the host clock around calls that end in a device synchronise, after a
warm-up, the smallest of REPS calls (and the median) -- REPS = 20 for the device, fewer for the host rules, as the lines say:
  (d) cocons_vecchia_group_device: host table in, labels out (upload, rounds, download and the plan statistics on the host);
  (h) cocons_vecchia_group_rounds, the same rule on one host thread;
  (g) cocons_vecchia_group, the greedy rule -- by this library and, with --parent-lib, by the library built from the parent
      commit, loaded beside this one;
  (k) cocons_fit_create_vecchia_grouped_knn, the whole handle on the device, against cocons_fit_create_vecchia_grouped fed with
      the finished table (the parent's route: greedy rule, expanded table, upload, set_groups);
and the rounds themselves by events (cocons_debug_group_rounds): live blocks and device time per round, the first rounds
against the tail.  Then the grouped value call and the grouped gradient call on the round rule's partition against the same
calls on the greedy partition, with blocks, rows per block and pairs per observation of both.  Nothing is asserted; the lines
also go to --out."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cocons_amd as ca                     # noqa: E402
from cocons_amd import _lib, host, workloads as wl     # noqa: E402


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
REPS = 20
FIRST = 12


def say(text):
    print(text, flush=True)
    LINES.append(text)


def finish():
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


def timed(fn, reps=REPS, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), 1e3 * float(np.median(ts))


def parent_greedy(path):
    L = ctypes.CDLL(path)
    ip = ctypes.POINTER(ctypes.c_int)
    L.cocons_vecchia_group.restype = ctypes.c_int
    L.cocons_vecchia_group.argtypes = [ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, ip, ctypes.POINTER(ctypes.c_longlong)]

    def call(nn):
        group = np.zeros(nn.shape[0], dtype=np.int32)
        assert L.cocons_vecchia_group(nn.shape[0], nn.shape[1], host._ip(nn), CAP, host._ip(group), None) == 0
        return group
    return call


def rounds_trace(nn):
    L = _lib.load()
    live = np.zeros(1024, dtype=np.int32)
    ms = np.zeros(1024)
    r = L.cocons_debug_group_rounds(nn.shape[0], nn.shape[1], host._ip(nn), CAP, 0, 0, 1024, host._ip(live), host._p(ms))
    assert r >= 1, _lib.last_error()
    return live[:r], ms[:r]                    # r: the rounds recorded


def partition_lines(name, st, n):
    return "%s: %d blocks, %.2f rows and %.2f members per block, %.1f pairs per observation (%.1f ungrouped)" % (
        name, st["blocks"], st["rows"] / st["blocks"], n / st["blocks"], st["pairs"] / n, st["pairs_ungrouped"] / n)


def calls(name, fit, th):
    tv = timed(lambda: fit.neg2loglik_core(th, grouped=True))
    tg = timed(lambda: fit.neg2loglik_grad_core(th, grouped=True))
    say("    %-28s grouped value %9.3f ms (median %9.3f), grouped value + gradient %9.3f ms (median %9.3f)" % ((name,) + tv + tg))


def one_order(n, name, locs, th, parent):
    host_reps = 3 if n <= 100000 else 1
    sc = wl.design_from_locs(locs)
    X, z = sc["std.covs"], wl.synthetic_z(n)
    nn = ca.vecchia_neighbours_device(locs, M)
    say("n = %d, m = %d, max_rows = %d, %s" % (n, M, CAP, name))
    keep = {}

    def kept(name, fn):
        def call():
            keep[name] = fn()
        return call

    td = timed(lambda: ca.vecchia_group_device(nn, CAP))
    gd, sd = ca.vecchia_group_device(nn, CAP, stats=True)
    th_ = timed(kept("h", lambda: ca.vecchia_group_rounds(nn, CAP, stats=True)), reps=host_reps, warm=False)
    gh, sh = keep["h"]
    tg = timed(kept("g", lambda: ca.vecchia_group(nn, CAP, stats=True)), reps=host_reps, warm=False)
    gg, sg = keep["g"]
    say("  (d) cocons_vecchia_group_device             %10.3f ms (median %10.3f), %d calls; %d rounds" % (td + (REPS, sd["rounds"])))
    say("  (h) cocons_vecchia_group_rounds, host       %10.3f ms (median %10.3f), %d call(s); the device's labels and rounds: %s" %
        (th_ + (host_reps, bool(np.array_equal(gd, gh) and sd == sh))))
    say("  (g) cocons_vecchia_group, greedy, host      %10.3f ms (median %10.3f), %d call(s)" % (tg + (host_reps,)))
    if parent:
        tp = timed(kept("p", lambda: parent(nn)), reps=host_reps, warm=False)
        say("  (g) the same by the parent commit's library %10.3f ms (median %10.3f); the same labels: %s" %
            (tp + (bool(np.array_equal(keep["p"], gg)),)))
    say("  (d) / (h) = %.4f, (d) / (g) = %.4f" % (td[0] / th_[0], td[0] / tg[0]))
    say("  " + partition_lines("round rule", sd, n))
    say("  " + partition_lines("greedy rule", sg, n))
    live, ms = rounds_trace(nn)
    k = min(FIRST, len(ms))
    say("  rounds by events: %d launched (the last finds no proposal); device time %.3f ms, of it %.3f ms in the first %d rounds and "
        "%.3f ms in the other %d" % (len(ms), float(ms.sum()), float(ms[:k].sum()), k, float(ms[k:].sum()), len(ms) - k))
    say("  live blocks at the start of each round: " + " ".join(map(str, live.tolist())))
    say("  ms per round: " + " ".join("%.3f" % v for v in ms))
    say("  scratch of the rounds: n (4 max_rows + 36) + 8 bytes = %.1f MB, beside the table's %.1f MB" %
        ((n * (4 * CAP + 36) + 8) / 1e6, n * M * 4 / 1e6))

    def knn_handle():
        ca.CoconsVecchiaFit.from_groups_knn(locs, X, z, wl.SMOOTH_LIMITS, M, max_rows=CAP).close()

    def table_handle():
        if "fg" in keep:
            keep.pop("fg").close()
        keep["fg"] = ca.CoconsVecchiaFit.from_groups(locs, X, z, wl.SMOOTH_LIMITS, nn, max_rows=CAP)

    tk = timed(knn_handle, reps=5)
    tt = timed(table_handle, reps=host_reps, warm=False)
    say("  (k) cocons_fit_create_vecchia_grouped_knn (search, rounds, plan, table, handle; destroyed) %10.3f ms (median %10.3f), 5 calls"
        % tk)
    say("  (k) cocons_fit_create_vecchia_grouped on the finished table (greedy; kept)                 %10.3f ms (median %10.3f), %d "
        "call(s)" % (tt + (host_reps,)))
    fr = ca.CoconsVecchiaFit.from_groups_knn(locs, X, z, wl.SMOOTH_LIMITS, M, max_rows=CAP)
    fg = keep.pop("fg")                        # (the last of the timed handles: it is not closed inside the timed stretch)
    say("  the handles: round rule m = %d, %.1f MB (plan %.2f MB); greedy rule m = %d, %.1f MB (plan %.2f MB)" %
        (fr.m, fr.info()["bytes"] / 1e6, fr.groups_info()["bytes"] / 1e6, fg.m, fg.info()["bytes"] / 1e6, fg.groups_info()["bytes"] / 1e6))
    calls("round rule's partition", fr, th)
    calls("greedy partition", fg, th)
    fr.close()
    fg.close()


say("python tools/vecchia_group_device_timing.py %s --m %d --max-rows %d%s" %
    (" ".join(map(str, SIZES)), M, CAP, " --parent-lib FILE" if PARENT else ""))
th = wl.theta_full()
ca.CoconsFit(np.random.default_rng(0).uniform(size=(300, 2)), np.ones((300, 1)), np.zeros(300), wl.SMOOTH_LIMITS).close()
parent = parent_greedy(PARENT) if PARENT else None
for n in SIZES:
    locs = np.random.default_rng(20260000 + n).uniform(0, 1, size=(n, 2))
    one_order(n, "random order", locs, th, parent)
    finish()
    order = ca.vecchia_order_device(locs).astype(np.int64) - 1
    one_order(n, "maxmin order", np.ascontiguousarray(locs[order]), th, parent)
    finish()
