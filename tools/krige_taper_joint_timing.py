"""Time the joint prediction of a tapered fit from the held band factor (cocons_krige_taper_joint) on a g x g
grid of observations with a Wendland-1 taper of range delta, at m prediction locations on a grid offset by half a cell:
    python tools/krige_taper_joint_timing.py [g=100] [delta=0.06] [m=4096] [nsim=64] [--calls K]
Reports prepare, then per ring depth D in {1, 2, 4, 8} (COCONS_KRIGE_JOINT_DEPTH) the wall time (min of 3) of the joint call
with cov only and with draws only, the largest drop of free device memory while a call runs and
cocons_krige_taper_joint_bytes; cov must come out the same bits at every depth.  --calls K: one prepare and K cov-only calls
at the default depth (for a kernel trace).  The lines are appended to profiles/krige_taper_joint_timing.txt (not with
--calls)."""
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cocons_amd as ca                     # noqa: E402
from cocons_amd import workloads as wl     # noqa: E402

CALLS = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
argv = [a for i, a in enumerate(sys.argv) if not a.startswith("--") and not (i > 0 and sys.argv[i - 1] == "--calls")]
g = int(argv[1]) if len(argv) > 1 else 100
delta = float(argv[2]) if len(argv) > 2 else 0.06
m = int(argv[3]) if len(argv) > 3 else 4096
nsim = int(argv[4]) if len(argv) > 4 else 64
n = g * g
DEPTHS = (1, 2, 4, 8)


def pattern(rows, cols, delta):
    """(colindices, rowpointers, entries), 1-based CSR, of the Wendland-1 taper between `rows` and `cols` (the cell buckets
    of tools/krige_taper_timing.py).  Columns ascend in a row."""
    key = lambda p: (np.floor(p[:, 0] / delta).astype(np.int64), np.floor(p[:, 1] / delta).astype(np.int64))   # noqa: E731
    ncell = int(np.ceil(max(rows.max(), cols.max()) / delta)) + 2
    cx, cy = key(cols)
    cid = (cx + 1) * (ncell + 2) + (cy + 1)
    order = np.argsort(cid, kind="stable")
    starts = np.searchsorted(cid[order], np.arange((ncell + 2) ** 2 + 1))
    rx, ry = key(rows)
    rid = (rx + 1) * (ncell + 2) + (ry + 1)
    rorder = np.argsort(rid, kind="stable")
    rstarts = np.searchsorted(rid[rorder], np.arange((ncell + 2) ** 2 + 1))
    R, C, E = [], [], []
    for c in np.unique(rid):
        ri = rorder[rstarts[c]:rstarts[c + 1]]
        cand = np.sort(np.concatenate([order[starts[c + a * (ncell + 2) + b]:starts[c + a * (ncell + 2) + b + 1]]
                                       for a in (-1, 0, 1) for b in (-1, 0, 1)]))
        if cand.size == 0:
            continue
        d = np.sqrt((rows[ri, 0][:, None] - cols[cand, 0][None, :]) ** 2 + (rows[ri, 1][:, None] - cols[cand, 1][None, :]) ** 2)
        a, b = np.nonzero(d <= delta)
        h = d[a, b] / delta
        R.append(ri[a]); C.append(cand[b]); E.append((1 - h) ** 4 * (4 * h + 1))
    R, C, E = np.concatenate(R), np.concatenate(C), np.concatenate(E)
    o = np.lexsort((C, R))
    rp = np.concatenate([[0], np.cumsum(np.bincount(R, minlength=rows.shape[0]))]) + 1
    return (C[o] + 1).astype(np.int32), rp.astype(np.int32), E[o]


def device_free_bytes():
    import ctypes
    from cocons_amd.shard import _hip_runtime
    hip = _hip_runtime()
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    return free.value


def watched(call):
    """(result, largest drop of free device memory while `call` ran)"""
    base = device_free_bytes()
    low, done = [base], threading.Event()

    def sample():
        while not done.is_set():
            low[0] = min(low[0], device_free_bytes())
            time.sleep(0.001)

    t = threading.Thread(target=sample)
    t.start()
    try:
        out = call()
    finally:
        done.set()
        t.join()
    return out, base - low[0]


locs = wl.grid_locs(g)
des = wl.design_from_locs(locs)
X = des["std.covs"]
th = wl.theta_full()
z = wl.synthetic_z(n)
gp = int(np.ceil(np.sqrt(m)))
lp = (wl.grid_locs(gp) * (1.0 - 1.0 / gp) + 0.5 / gp)[:m]          # a gp x gp grid of cell centres: half a cell off the border
Xp = wl.design_from_locs(lp, des["mean.vector"], des["sd.vector"])["std.covs"]
t0 = time.perf_counter()
ref_taper = pattern(locs, locs, delta)
pred_taper = pattern(lp, locs, delta)
uu_taper = pattern(lp, lp, delta)
E = np.random.default_rng(1).standard_normal((m, nsim))
lines = ["python tools/krige_taper_joint_timing.py %d %g %d %d" % (g, delta, m, nsim),
         "n = %d, delta = %g, nnz = %d (%.1f per row); m = %d, nnz_pred = %d (%.1f per row), nnz_uu = %d (%.1f per row); "
         "patterns built in %.1f s" % (n, delta, ref_taper[0].size, ref_taper[0].size / n, m, pred_taper[0].size,
                                       pred_taper[0].size / m, uu_taper[0].size, uu_taper[0].size / m, time.perf_counter() - t0)]
print(lines[-1], flush=True)
fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
fit.krige_taper_prepare(th)
tp = []
for _ in range(3):
    t0 = time.perf_counter(); fit.krige_taper_prepare(th); tp.append(time.perf_counter() - t0)
info = fit.krige_taper_info()
os.environ.pop("COCONS_KRIGE_JOINT_DEPTH", None)
if CALLS:
    for _ in range(CALLS):
        fit.krige_taper_joint_core(lp, Xp, pred_taper, uu_taper)
    sys.exit(0)
lines.append("prepare: %.1f ms (min of 3); state %.3f GB, W = %d of nt = %d tile columns" %
             (1e3 * min(tp), info["bytes"] / 1e9, info["W"], info["nt"]))
print(lines[-1], flush=True)
lines.append("%5s %12s %14s %14s %12s" % ("D", "cov only ms", "draws only ms", "mem drop GB", "bytes GB"))
first = None
for D in DEPTHS:
    os.environ["COCONS_KRIGE_JOINT_DEPTH"] = str(D)
    (st, cov, _), drop = watched(lambda: fit.krige_taper_joint_core(lp, Xp, pred_taper, uu_taper))
    if first is None:
        first = cov
    same = bool(np.array_equal(cov, first))
    tc, td = [], []
    for _ in range(3):
        t0 = time.perf_counter(); fit.krige_taper_joint_core(lp, Xp, pred_taper, uu_taper); tc.append(time.perf_counter() - t0)
    fit.krige_taper_joint_core(lp, Xp, pred_taper, uu_taper, iiderrors=E, cov=False)
    for _ in range(3):
        t0 = time.perf_counter()
        fit.krige_taper_joint_core(lp, Xp, pred_taper, uu_taper, iiderrors=E, cov=False)
        td.append(time.perf_counter() - t0)
    lines.append("%5d %12.1f %14.1f %14.3f %12.3f   cov-only runs %s, draws-only runs %s%s" %
                 (D, 1e3 * min(tc), 1e3 * min(td), drop / 1e9, fit.krige_taper_joint_bytes(m, nsim) / 1e9,
                  " ".join("%.1f" % (1e3 * t) for t in tc), " ".join("%.1f" % (1e3 * t) for t in td),
                  "" if same else "   COV DIFFERS FROM D = 1"))
    print(lines[-1], flush=True)
npad = info["nt"] * 128
lines.append("Schur flops m^2 npad = %.3e; a buffer of round_up(m, 64) x npad would be %.3f GB" %
             (float(m) * m * npad, 8.0 * ((m + 63) // 64 * 64) * npad / 1e9))
print(lines[-1], flush=True)
fit.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "krige_taper_joint_timing.txt"), "a") as fh:
    fh.write("\n".join(lines) + "\n\n")
