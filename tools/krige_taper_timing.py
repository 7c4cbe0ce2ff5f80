"""Time tapered kriging from a held band factor (cocons_krige_taper_prepare / _apply) on a g x g grid of
observations with a Wendland-1 taper of range delta, at m prediction locations on a grid offset by half a cell:
    python tools/krige_taper_timing.py [g=100] [delta=0.06] [m=65536] [--oneshot] [--calls K]
Reports prepare (ms), apply (ms and per row), the state's bytes, W and rows per chunk.  --oneshot: also the one-shot
route cocons_predict_taper in slices of the same number of rows -- time per row and the drop of free device memory.
--calls K: one prepare and K applies only (for a kernel trace).  The lines are appended to profiles/krige_taper_timing.txt
(not with --calls)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cocons_amd as ca                     # noqa: E402
from cocons_amd import workloads as wl     # noqa: E402

FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
CALLS = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
argv = [a for i, a in enumerate(sys.argv) if not a.startswith("--") and not (i > 0 and sys.argv[i - 1] == "--calls")]
g = int(argv[1]) if len(argv) > 1 else 100
delta = float(argv[2]) if len(argv) > 2 else 0.06
m = int(argv[3]) if len(argv) > 3 else 65536
n = g * g


def pattern(rows, cols, delta):
    """(colindices, rowpointers, entries), 1-based CSR, of the Wendland-1 taper between `rows` and `cols`: the cell
    buckets of tools/taper_timing.py, a cell's rows against the 3 x 3 cells around it at once.  Columns ascend in a row."""
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
lines = ["python tools/krige_taper_timing.py %d %g %d%s" % (g, delta, m, " --oneshot" if "--oneshot" in FLAGS else ""),
         "n = %d, delta = %g, nnz = %d (%.1f per row); m = %d, nnz_pred = %d (%.1f per row); patterns built in %.1f s" %
         (n, delta, ref_taper[0].size, ref_taper[0].size / n, m, pred_taper[0].size, pred_taper[0].size / m,
          time.perf_counter() - t0)]
print(lines[-1], flush=True)
fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
fit.neg2loglik_core(th)
t0 = time.perf_counter(); fit.neg2loglik_core(th); t_obj = time.perf_counter() - t0
fit.krige_taper_prepare(th)
t0 = time.perf_counter(); fit.krige_taper_prepare(th); t_prep = time.perf_counter() - t0
info = fit.krige_taper_info()
if CALLS:
    for _ in range(CALLS):
        fit.krige_taper_core(lp, Xp, pred_taper)
    sys.exit(0)
st, qf = fit.krige_taper_core(lp, Xp, pred_taper)
ta = []
for _ in range(2):
    t0 = time.perf_counter(); st2, qf2 = fit.krige_taper_core(lp, Xp, pred_taper); ta.append(time.perf_counter() - t0)
t_app = min(ta)
lines.append("objective (one factorisation): %.1f ms; prepare: %.1f ms" % (1e3 * t_obj, 1e3 * t_prep))
lines.append("apply, m = %d: %.1f ms, %.2f us per row (a repeat: no factorisation; same bits: %s)" %
             (m, 1e3 * t_app, 1e6 * t_app / m, bool(np.array_equal(st, st2) and np.array_equal(qf, qf2))))
lines.append("state: %.3f GB, W = %d of nt = %d tile columns, %d rows per chunk" %
             (info["bytes"] / 1e9, info["W"], info["nt"], info["rows"]))
print("\n".join(lines[1:]), flush=True)
if "--oneshot" in FLAGS:
    rows = info["rows"]
    fit.krige_taper_release()
    ci, rp, ent = pred_taper
    free0 = device_free_bytes()
    low = free0
    out_st, out_qf = np.empty(m), np.empty(m)
    tt = 0.0
    for rep in range(2):                      # the first pass grows the handle's buffer; the second is timed
        t0 = time.perf_counter()
        for b in range(0, m, rows):
            e = min(b + rows, m)
            sl = (ci[rp[b] - 1:rp[e] - 1], rp[b:e + 1] - rp[b] + 1, ent[rp[b] - 1:rp[e] - 1])
            out_st[b:e], out_qf[b:e] = fit.predict_core(th, lp[b:e], Xp[b:e], sl)
            low = min(low, device_free_bytes())
        tt = time.perf_counter() - t0
    err = max(float(np.max(np.abs(st - out_st)) / np.max(np.abs(out_st))), float(np.max(np.abs(qf - out_qf)) / np.max(np.abs(out_qf))))
    lines.append("one-shot route in slices of %d rows: %.1f ms, %.2f us per row; free device memory dropped by %.3f GB; "
                 "largest difference between the routes %.2e of the largest value" %
                 (rows, 1e3 * tt, 1e6 * tt / m, (free0 - low) / 1e9, err))
    lines.append("time per row, held band factor / sliced one-shot: %.3f" % (t_app / tt))
    print("\n".join(lines[-2:]), flush=True)
fit.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "krige_taper_timing.txt"), "a") as fh:
    fh.write("\n".join(lines) + "\n\n")
