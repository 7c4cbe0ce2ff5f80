#!/usr/bin/env python3
"""Joint prediction from a held factor (cocons_krige_joint): wall time and drop of free device memory of
  * cocons_krige_prepare,
  * the joint call with cov only,
  * the joint call with 64 draws and no cov,
  * the one-shot cocons_sim_cond_dense with the same 64 draws (the joint (n + m) factorisation),
at n = m = 8192 (config C5: the 128 x 64 grid and the half-cell-shifted grid of tools/krige_timing.py) and at n = 10^4,
m = 4096 (uniform locations).  Wall times here; the device time of krige_schur_kernel comes from one run of this tool under
rocprofv3 --kernel-trace --stats (no counters in that run), turned into a rate of m^2 npad flops.
Prints and writes profiles/krige_joint_timing.txt.  usage: tools/krige_joint_timing.py [--sizes c5,4096] [--reps 3]"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cocons_amd as ca  # noqa: E402
from cocons_amd import workloads as wl  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from krige_timing import free_bytes, problem  # noqa: E402

NSIM = 64


def timed(fn, reps):
    """(min wall seconds, largest drop of free device memory while fn runs, last result)"""
    best, low = float("inf"), [free_bytes()]
    base = low[0]
    for _ in range(reps):
        done = threading.Event()

        def sample():
            while not done.is_set():
                low[0] = min(low[0], free_bytes())
                time.sleep(0.001)

        t = threading.Thread(target=sample)
        t.start()
        try:
            t0 = time.perf_counter()
            out = fn()
            best = min(best, time.perf_counter() - t0)
        finally:
            done.set()
            t.join()
    return best, base - low[0], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="c5,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krige_joint_timing.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for size in a.sizes.split(","):
        locs, X, z, th, lp, Xp = problem(size)
        n, m = locs.shape[0], lp.shape[0]
        npad = (n + 127) // 128 * 128
        E = np.random.default_rng(9).standard_normal((m, NSIM))
        fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
        fit.neg2loglik_core(th)                  # warm: the handle's own buffers and the engine
        t_prep, d_prep, _ = timed(lambda: fit.krige_prepare(th), a.reps)
        fit.krige_joint_core(lp[:256], Xp[:256], iiderrors=E[:256])      # warm: the hand-off scratch of a view's factorisation
        t_cov, d_cov, (st, cov, _) = timed(lambda: fit.krige_joint_core(lp, Xp), a.reps)
        t_sim, d_sim, (_, _, sims) = timed(lambda: fit.krige_joint_core(lp, Xp, iiderrors=E, cov=False), a.reps)
        assert np.array_equal(cov, cov.T) and np.all(np.isfinite(sims))
        del cov
        fit.krige_release()
        t_one, d_one, want = timed(lambda: fit.sim_cond_core(th, lp, Xp, lp, E), a.reps)
        fit.close()
        d = np.max(np.abs(sims - want)) / np.max(np.abs(want))
        say("krige_joint n=%d m=%d (npad %d, %d draws, min of %d):" % (n, m, npad, NSIM, a.reps))
        say("  prepare                      %9.2f ms   free memory drop %.3f GB" % (1e3 * t_prep, d_prep / 1e9))
        say("  joint, cov only              %9.2f ms   free memory drop %.3f GB   (m^2 npad = %.3g flops in the Schur product)"
            % (1e3 * t_cov, d_cov / 1e9, float(m) * m * npad))
        say("  joint, %d draws, no cov      %9.2f ms   free memory drop %.3f GB" % (NSIM, 1e3 * t_sim, d_sim / 1e9))
        say("  cocons_sim_cond_dense        %9.2f ms   free memory drop %.3f GB   (one-shot: factors n + m = %d)"
            % (1e3 * t_one, d_one / 1e9, n + m))
        say("  prepare + joint draws        %9.2f ms   max rel. difference of the draws to the one-shot entry %.2e"
            % (1e3 * (t_prep + t_sim), d))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
