#!/usr/bin/env python3
"""Kriging from a held factor (cocons_krige_prepare / _apply): wall and device time of prepare and apply, and the drop
in free device memory, at
  * n = m = 8192 (config C5: the 128 x 64 grid and the half-cell-shifted grid of tools/predict_timing.py),
  * n = 10^4, m = 65 536 and n = 10^4, m = 10^6 (uniform locations),
with cocons_predict_dense beside it where its bordered buffer fits.  Wall times here; the device time of every kernel
comes from a run under rocprofv3 --kernel-trace --stats (profiles/krige_*_kernel_stats.csv).  usage: tools/krige_timing.py [--sizes c5,65536,1e6] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca  # noqa: E402
from cocons_amd import workloads as wl  # noqa: E402

PEAK_F64_MFMA = 78.6e12


def free_bytes():
    """Free device memory (hipMemGetInfo)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def problem(size):
    th = wl.theta_full()
    th["mean"] = np.array([0.3, -0.1, 0.2])
    if size == "c5":
        locs = wl.grid_locs(128, 64)
        sc = wl.design_from_locs(locs)
        lp = locs + np.array([0.5 / 127, 0.5 / 63])
        Xp = wl.design_from_locs(lp, sc["mean.vector"], sc["sd.vector"])["std.covs"]
        return locs, sc["std.covs"], wl.synthetic_z(8192), th, lp, Xp
    m = int(float(size))
    rng = np.random.default_rng(5)
    n = 10_000
    locs = rng.uniform(0, 1, size=(n, 2))
    sc = wl.design_from_locs(locs)
    lp = rng.uniform(0, 1, size=(m, 2))
    Xp = wl.design_from_locs(lp, sc["mean.vector"], sc["sd.vector"])["std.covs"]
    return locs, sc["std.covs"], wl.synthetic_z(n), th, lp, Xp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="c5,65536,1e6")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for size in a.sizes.split(","):
        locs, X, z, th, lp, Xp = problem(size)
        n, m = locs.shape[0], lp.shape[0]
        fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
        fit.neg2loglik_core(th)                  # warm: the handle's own buffers and the engine
        free_base = free_bytes()
        prep = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fit.krige_prepare(th)
            prep.append(time.perf_counter() - t0)
        info = fit.krige_info()
        free_prepared = free_bytes()
        reps = a.reps if m <= 100_000 else 1
        app = []
        for _ in range(reps):
            t0 = time.perf_counter()
            st, qf = fit.krige_core(lp, Xp)
            app.append(time.perf_counter() - t0)
        free_after = free_bytes()
        flops = float(n) * n * m
        line = ("krige n=%d m=%d: prepare %.2f ms (min of %d), apply %.2f ms (min of %d) = %.1f TFLOP/s on n^2 m (%.0f %% of "
                "fp64 MFMA peak); state %.3f GB, %d rows per chunk; free memory drop: prepared %.3f GB, after apply %.3f GB"
                % (n, m, 1e3 * min(prep), len(prep), 1e3 * min(app), len(app), flops / min(app) / 1e12,
                   100 * flops / min(app) / PEAK_F64_MFMA, info["bytes"] / 1e9, info["rows"],
                   (free_base - free_prepared) / 1e9, (free_base - free_after) / 1e9))
        print(line, flush=True)
        assert np.all(np.isfinite(st)) and np.all(np.isfinite(qf))
        bordered = 8.0 * (n + m + 256) * n * 2           # dA grown to m + 1 rows under the matrix, and the DAG's second buffer
        if bordered < 0.5 * free_bytes():
            fit.krige_release()
            fit.predict_core(th, lp, Xp)
            pts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                st2, qf2 = fit.predict_core(th, lp, Xp)
                pts.append(time.perf_counter() - t0)
            d = max(np.max(np.abs(st - st2)) / np.max(np.abs(st2)), np.max(np.abs(qf - qf2) / np.abs(qf2)))
            print("  cocons_predict_dense n=%d m=%d: %.2f ms (min of %d; factorisation + solve); free memory drop %.3f GB; "
                  "max rel. difference to krige %.2e" % (n, m, 1e3 * min(pts), len(pts),
                                                          (free_base - free_bytes()) / 1e9, d), flush=True)
        else:
            print("  cocons_predict_dense n=%d m=%d: not run (its bordered buffers need about %.0f GB)" % (n, m, bordered / 1e9),
                  flush=True)
        fit.close()


if __name__ == "__main__":
    main()
