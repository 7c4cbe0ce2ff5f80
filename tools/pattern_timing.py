"""Time the taper-pattern builder (cocons_taper_pattern, cocons_krige_taper_apply_delta) against the host route
on a g x g grid of observations with a Wendland-1 taper of range delta and m prediction locations on a grid offset by
half a cell (the cases of tools/krige_taper_timing.py):
    python tools/pattern_timing.py [g=100] [delta=0.06] [m=65536]
(a) the self pattern: cocons_amd.taper_pattern (count call + fill call, host buffers in and out) against scipy's cKDTree
    with 16 threads (query_ball_point, sorted) plus the CSR and the entries in numpy;
(b) kriging at the m locations from one prepared state: krige_taper_core_delta end to end against the host route --
    the cKDTree pattern, then krige_taper_core (host bucketing, uploads and the device solve in one call).
Every timed call is warmed up once and repeated; the minimum and the median of the repeats are reported.  The lines are
appended to profiles/pattern_timing.txt.
    python tools/pattern_timing.py g delta m --calls K         one prepare and K krige_taper_core_delta calls only, for
                                                              rocprofv3 --kernel-trace --stats (a run of its own)
    python tools/pattern_timing.py g delta m --stats CSV K     append the kernel split of that run's kernel_stats CSV
                                                              (per call: the builder's kernels, the solve's), and with
                                                              it the split of the two routes of (b) measured before"""
import csv
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "pattern_timing.txt")
THREADS = 16
REPS = 5

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
mode = next((a for a in sys.argv[1:] if a.startswith("--")), "")
g = int(pos[0]) if len(pos) > 0 else 100
delta = float(pos[1]) if len(pos) > 1 else 0.06
m = int(pos[2]) if len(pos) > 2 else 65536
n = g * g
tag = "g = %d (n = %d), delta = %g, m = %d" % (g, n, delta, m)


def append(lines):
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as fh:
        fh.write("\n".join(lines) + "\n\n")


if mode == "--stats":
    path, calls = pos[3], int(pos[4])
    groups = {"builder": 0.0, "solve": 0.0}
    rows = []
    for r in csv.DictReader(open(path)):
        name, tot = r["Name"], float(r["TotalDurationNs"]) / calls * 1e-6
        if "pattern_" in name or "scan_exclusive" in name:
            groups["builder"] += tot
            rows.append("    %-32s %6d calls  %9.3f ms per apply" % (re.search(r"(\w+_kernel)", name).group(1), int(r["Calls"]) // calls, tot))
        elif "krige_band" in name or "taper" in name or "loc_params" in name:
            groups["solve"] += tot
    lines = ["kernel split of krige_taper_core_delta (rocprofv3 --kernel-trace --stats, %d calls), %s" % (calls, tag)] + rows
    lines.append("    builder kernels %.3f ms, entry and ring-solve kernels %.3f ms per apply" % (groups["builder"], groups["solve"]))
    wall = {}
    if os.path.exists(OUT):                      # the walls of (b), written by the plain run of the same case
        for line in open(OUT):
            if line.startswith("(b) ") and tag in line:
                wall = dict(kv.split("=") for kv in line.split("|")[1].split())
    if wall:
        host_apply, search, dl = float(wall["host_apply_ms"]), float(wall["host_search_ms"]), float(wall["delta_ms"])
        lines.append("    host route : search %.1f ms | rest of the call (host bucketing, uploads, launches) %.1f ms (apply %.1f - solve kernels) | device solve %.1f ms"
                     % (search, host_apply - groups["solve"], host_apply, groups["solve"]))
        lines.append("    delta route: search %.1f ms (builder kernels) | rest of the call (launches, the offsets' wait) %.1f ms | device solve %.1f ms"
                     % (groups["builder"], dl - groups["builder"] - groups["solve"], groups["solve"]))
    append(lines)
    sys.exit(0)

import cocons_amd as ca                     # noqa: E402
from cocons_amd import workloads as wl     # noqa: E402


def timed(f, reps=REPS):
    f()                                      # warm-up: code objects, allocations, the state's grid and staging
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = f(); ts.append(time.perf_counter() - t0)
    return out, 1e3 * min(ts), 1e3 * float(np.median(ts))


def kdtree_pattern(rows, cols, delta):
    """(colindices, rowpointers, entries) by cKDTree on the host; returns the pattern and the seconds of the search alone"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    nb = cKDTree(cols).query_ball_point(rows, delta, workers=THREADS, return_sorted=True)
    t_search = time.perf_counter() - t0
    cnt = np.fromiter((len(v) for v in nb), dtype=np.int64, count=len(nb))
    ci = np.concatenate([np.asarray(v, dtype=np.int64) for v in nb]) if cnt.sum() else np.zeros(0, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(cnt)]) + 1
    ri = np.repeat(np.arange(rows.shape[0]), cnt)
    dx, dy = rows[ri, 0] - cols[ci, 0], rows[ri, 1] - cols[ci, 1]
    h = np.sqrt(dx * dx + dy * dy) / delta
    u2 = (1 - h) * (1 - h)
    return ((ci + 1).astype(np.int32), rp.astype(np.int32), (u2 * u2) * (4 * h + 1)), t_search


locs = wl.grid_locs(g)
des = wl.design_from_locs(locs)
X = des["std.covs"]
th = wl.theta_full()
z = wl.synthetic_z(n)
gp = int(np.ceil(np.sqrt(m)))
lp = (wl.grid_locs(gp) * (1.0 - 1.0 / gp) + 0.5 / gp)[:m]          # cell centres: half a cell off the border
Xp = wl.design_from_locs(lp, des["mean.vector"], des["sd.vector"])["std.covs"]

if mode == "--calls":
    K = int(pos[3])
    fit = ca.CoconsTaperFit.from_delta(locs, X, z, wl.SMOOTH_LIMITS, delta, "wend1")
    fit.krige_taper_prepare(th)
    for _ in range(K):
        fit.krige_taper_core_delta(lp, Xp, delta, "wend1")
    fit.close()
    sys.exit(0)

lines = ["python tools/pattern_timing.py %d %g %d" % (g, delta, m)]
# (a) the self pattern
dev, a_min, a_med = timed(lambda: ca.taper_pattern(locs, delta, "wend1"))
(host, _), h_min, h_med = timed(lambda: kdtree_pattern(locs, locs, delta), reps=3)
same = bool(np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]))
lines.append("(a) self pattern, %s: nnz = %d (%.1f per row); cocons_taper_pattern %.1f ms (median %.1f); cKDTree x%d + CSR + entries "
             "%.1f ms (median %.1f); same pattern: %s, largest entry difference %.2e"
             % (tag, dev[0].size, dev[0].size / n, a_min, a_med, THREADS, h_min, h_med, same,
                float(np.max(np.abs(dev[2] - host[2]))) if same else float("nan")))
print(lines[-1], flush=True)
# (b) kriging by both routes from one prepared state
fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *dev)
fit.krige_taper_prepare(th)
info = fit.krige_taper_info()
got, d_min, d_med = timed(lambda: fit.krige_taper_core_delta(lp, Xp, delta, "wend1"))
(pred, t_search), p_min, p_med = timed(lambda: kdtree_pattern(lp, locs, delta), reps=3)
want, ap_min, ap_med = timed(lambda: fit.krige_taper_core(lp, Xp, pred))
bits = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
lines.append("(b) kriging, %s: nnz_pred = %d (%.1f per row), %d rows per chunk, state %.3f GB | delta_ms=%.1f host_search_ms=%.1f "
             "host_apply_ms=%.1f | krige_taper_core_delta %.1f ms (median %.1f); host route %.1f ms = cKDTree pattern %.1f "
             "(median %.1f; the tree search alone %.1f) + krige_taper_core %.1f (median %.1f); same bits: %s"
             % (tag, fit.last_pattern_nnz, fit.last_pattern_nnz / m, info["rows"], fit.krige_taper_info()["bytes"] / 1e9,
                d_min, p_min, ap_min, d_min, d_med, p_min + ap_min, p_min, p_med, 1e3 * t_search, ap_min, ap_med, bits))
fit.close()
append(lines)
