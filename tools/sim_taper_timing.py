"""Time the sparse branch of cocoSim (cocons_sim_taper: assembly + band-limited factorisation + band_trmm_kernel) on a
g x g grid with a Wendland-1 taper of range delta (the pattern builder of tools/taper_timing.py):
    python tools/sim_taper_timing.py [g=100] [delta=0.06] [nsim list=1,16,64,256]
Per nsim: total call time (host clock around the call, which ends in a device synchronise) and the device-event times of
its stages (assembly + factorisation, band product, gather into the caller's order); the bytes the product must read --
envelope tiles x 128^2 x 8 B x ceil(nsim / 64) -- and the rate that makes against the 6.3 TB/s of HBM."""
import ctypes
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca                     # noqa: E402
from cocons_amd import _lib                 # noqa: E402
from cocons_amd import workloads as wl     # noqa: E402

HBM_BPS = 6.3e12
g = int(sys.argv[1]) if len(sys.argv) > 1 else 100
delta = float(sys.argv[2]) if len(sys.argv) > 2 else 0.06
nsims = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64, 256]
n = g * g
locs = wl.grid_locs(g)
X = wl.design_from_locs(locs)["std.covs"]
th = wl.theta_full()
th["mean"] = np.array([0.3, -0.2, 0.1])
z = wl.synthetic_z(n)
t0 = time.perf_counter()
ci, rp, ent = [], [1], []
cell = {}
for i, (x, y) in enumerate(locs):
    cell.setdefault((int(x / delta), int(y / delta)), []).append(i)
for i, (x, y) in enumerate(locs):
    cx, cy = int(x / delta), int(y / delta)
    cand = np.array(sorted(j for a in (-1, 0, 1) for b in (-1, 0, 1) for j in cell.get((cx + a, cy + b), [])))
    d = np.sqrt(np.sum((locs[cand] - locs[i]) ** 2, axis=1))
    keep = d <= delta
    h = d[keep] / delta
    ci.extend((cand[keep] + 1).tolist())
    ent.extend(((1 - h) ** 4 * (4 * h + 1)).tolist())
    rp.append(len(ci) + 1)
ci, rp, ent = np.array(ci, dtype=np.int32), np.array(rp, dtype=np.int32), np.array(ent)
print("pattern: n = %d, delta = %g, nnz = %d (%.1f per row), built in %.1f s" %
      (n, delta, ci.size, ci.size / n, time.perf_counter() - t0))

L = _lib.load()
ca.CoconsFit(locs[:300], X[:300], z[:300], wl.SMOOTH_LIMITS).neg2loglik_core(th)     # library + context are up
t0 = time.perf_counter()
fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, ent)
L.cocons_fit_sync(fit._h)
print("handle creation: %.1f ms" % (1e3 * (time.perf_counter() - t0)))
fit.neg2loglik_core(th)
t0 = time.perf_counter()
K = 5
for _ in range(K):
    fit.neg2loglik_core(th)
print("taper objective (one evaluation, for comparison): %.2f ms" % (1e3 * (time.perf_counter() - t0) / K))
rng = np.random.default_rng(1)
st = (ctypes.c_double * 4)()
print("%6s %10s %12s %12s %10s %12s %10s %8s" % ("nsim", "total ms", "assm+fact ms", "product ms", "gather ms",
                                                   "band GB read", "GB/s", "of HBM"))
for nsim in nsims:
    E = rng.standard_normal((n, nsim))
    fit.sim_core(th, E)                           # warm-up of this shape
    reps = 5
    tot, parts = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fit.sim_core(th, E)
        tot.append(time.perf_counter() - t0)
        _lib.check(L.cocons_debug_sim_taper_ms(fit._h, 0, st), "cocons_debug_sim_taper_ms")
        parts.append(list(st))
    parts = np.median(np.array(parts), axis=0)
    tiles = parts[3]
    band = tiles * 128 * 128 * 8 * math.ceil(nsim / 64)
    rate = band / (parts[1] * 1e-3)
    print("%6d %10.2f %12.2f %12.3f %10.3f %12.3f %10.0f %7.1f%%" % (nsim, 1e3 * np.median(tot), parts[0], parts[1], parts[2],
                                                                     band / 1e9, rate / 1e9, 100 * rate / HBM_BPS))
print("envelope: %d tiles of 128 x 128 (%.3f GB) of %d in the lower triangle" % (tiles, tiles * 128 * 128 * 8 / 1e9,
                                                                               fit.n // 128 * (fit.n // 128 + 1) // 2))
fit.close()
