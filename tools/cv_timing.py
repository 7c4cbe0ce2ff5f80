#!/usr/bin/env python3
"""Cross-validated predictions from one factorisation (cocons_cv_dense / cocons_cv_taper): best-of-reps wall time
of the host call on ONE handle, at n = 4096 and n = 10^4 (the grid problems of bench.py's C2 / C3, the C4 model's theta):
  loo        one leave-one-out call (fold = None);
  fold10     one call with 10 random folds of equal size;
  block100   one call with 100 spatial blocks (10 x 10);
  grad       one neg2loglik_grad_core call on the same handle;
  refit10    the route a caller had before: per fold a fresh CoconsFit on the complement plus predict_core at the fold's sites,
             handle creation included.
Conditions: fold10 < refit10; loo <= 1.1 grad.
With --taper: leave-one-out on a taper handle against the taper gradient call on the same handle, at n = 10^4 (delta = 0.06)
and n = 99 856 (delta = 0.019).
With --taper-folds: cross-validation by folds on the held band factor (cocons_cv_taper_folds) on the same two taper problems,
one handle, every shape warmed up, each call ending in a synchronise (the call returns host arrays):
  size10     n / 10 random folds of 10 observations;   block100   100 spatial blocks;   fold10   10 random folds;
  loo        the leave-one-out call on the same handle;   *_bytes   the device bytes of the call (stats5[4]);
  (--fold-counts 15,20: k random folds of n / k instead of the three cases -- where the two routes cross)
  refit_*    the route a caller had before: per fold a fresh CoconsTaperFit on the complement plus predict_core at the fold's
             sites, handle creation included, the sub-patterns cut on the host beforehand -- timed on --refit-folds folds
             (default 3, the first labels) and scaled to the number of folds.
With --stages-only N [--mode loo|fold10|block100]: only such calls (for a run under rocprofv3 --kernel-trace --stats); with
--taper-folds it takes the first of --taper-grids.
One JSON line.
usage: tools/cv_timing.py [--taper | --taper-folds] [--sizes 4096,10000] [--reps 5] [--out FILE] [--stages-only N --mode M]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca  # noqa: E402
from cocons_amd import workloads as wl  # noqa: E402


def problem(n):
    g = int(round(np.sqrt(n)))
    locs = wl.grid_locs(g, n // g) if g * (n // g) == n else np.random.default_rng(1).uniform(0, 1, size=(n, 2))
    X = wl.design_from_locs(locs)["std.covs"]
    return locs, X, wl.synthetic_z(n)


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def fold_labels(locs, mode):
    n = locs.shape[0]
    if mode == "loo":
        return None
    if mode == "fold10":
        return np.random.default_rng(7).permutation(n) % 10
    lo, hi = locs.min(axis=0), locs.max(axis=0)
    cell = np.minimum(((locs - lo) / (hi - lo) * 10).astype(int), 9)
    return cell[:, 0] * 10 + cell[:, 1]


def refit(th, locs, X, z, lab):
    """every fold predicted from a fresh handle on its complement"""
    out = np.empty(locs.shape[0])
    for l in np.unique(lab):
        B, A = lab == l, lab != l
        f = ca.CoconsFit(locs[A], X[A], z[A], wl.SMOOTH_LIMITS)
        try:
            st, _ = f.predict_core(th, locs[B], X[B])
        finally:
            f.close()
        out[B] = st
    return out


def time_size(n, reps):
    locs, X, z = problem(n)
    th = wl.theta_full()
    lab10, lab100 = fold_labels(locs, "fold10"), fold_labels(locs, "block100")
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        out = {"n": n,
               "grad_ms": best(lambda: fit.neg2loglik_grad_core(th), reps),
               "loo_ms": best(lambda: fit.cv_core(th), reps),
               "fold10_ms": best(lambda: fit.cv_core(th, lab10), reps),
               "block100_ms": best(lambda: fit.cv_core(th, lab100), reps),
               "block100_sizes": [int(np.bincount(lab100).min()), int(np.bincount(lab100).max())]}
        resid, _ = fit.cv_core(th, lab10)
    finally:
        fit.close()
    out["refit10_ms"] = best(lambda: refit(th, locs, X, z, lab10), max(1, reps // 2))
    st = refit(th, locs, X, z, lab10)
    R = z.reshape(n, -1)[:, 0] - X @ th["mean"]
    out["fold10_vs_refit_max_abs"] = float(np.max(np.abs(resid[:, 0] - (R - st))))
    out["loo_over_grad"] = out["loo_ms"] / out["grad_ms"]
    out["fold10_over_refit10"] = out["fold10_ms"] / out["refit10_ms"]
    out["loo_within_10_percent_of_grad"] = bool(out["loo_ms"] <= 1.1 * out["grad_ms"])
    out["fold10_cheaper_than_refit10"] = bool(out["fold10_ms"] < out["refit10_ms"])
    return out


def wendland1_pattern(locs, delta):
    """(colindices, rowpointers, entries) of the Wendland-1 taper (1 - h)^4 (4 h + 1), h = d / delta <= 1: 1-based CSR"""
    from scipy.spatial import cKDTree
    n = locs.shape[0]
    pairs = cKDTree(locs).query_pairs(delta, output_type="ndarray")
    i = np.concatenate([pairs[:, 0], pairs[:, 1], np.arange(n)])
    j = np.concatenate([pairs[:, 1], pairs[:, 0], np.arange(n)])
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    h = np.sqrt(np.sum((locs[i] - locs[j]) ** 2, axis=1)) / delta
    rp = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))]) + 1
    return (j + 1).astype(np.int32), rp.astype(np.int32), (1 - h) ** 4 * (4 * h + 1)


def time_taper(g, delta, reps):
    n = g * g
    locs = wl.grid_locs(g)
    X = wl.design_from_locs(locs)["std.covs"]
    z = wl.synthetic_z(n)
    th = wl.theta_full()
    ref_taper = wendland1_pattern(locs, delta)
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
    try:
        out = {"n": n, "delta": delta, "nnz": int(ref_taper[0].size),
               "grad_ms": best(lambda: fit.neg2loglik_grad_core(th), reps),
               "loo_ms": best(lambda: fit.cv_core(th), reps)}
    finally:
        fit.close()
    out["loo_over_grad"] = out["loo_ms"] / out["grad_ms"]
    out["loo_within_10_percent_of_grad"] = bool(out["loo_ms"] <= 1.1 * out["grad_ms"])
    return out


def taper_problem(g, delta):
    locs = wl.grid_locs(g)
    return locs, wl.design_from_locs(locs)["std.covs"], wl.synthetic_z(g * g), wendland1_pattern(locs, delta)


def size10_labels(n):
    return np.random.default_rng(9).permutation(n) // 10


def refit_taper(th, locs, X, z, ref_taper, lab, nfolds):
    """(seconds for the first nfolds folds, largest |difference| to `check` is the caller's): every fold predicted from a fresh
    taper handle on its complement; the sub-patterns are cut before the clock starts"""
    from scipy.sparse import csr_matrix
    n = locs.shape[0]
    ci, rp, ent = ref_taper
    T = csr_matrix((ent, ci - 1, rp - 1), shape=(n, n))
    cut = []
    for l in np.unique(lab)[:nfolds]:
        B, A = np.nonzero(lab == l)[0], np.nonzero(lab != l)[0]
        TA, TB = T[A][:, A].tocsr(), T[B][:, A].tocsr()
        TA.sort_indices(); TB.sort_indices()
        cut.append((A, B, ((TA.indices + 1).astype(np.int32), (TA.indptr + 1).astype(np.int32), TA.data),
                    ((TB.indices + 1).astype(np.int32), (TB.indptr + 1).astype(np.int32), TB.data)))
    out = {}
    t0 = time.perf_counter()
    for A, B, tA, tB in cut:
        f = ca.CoconsTaperFit(locs[A], X[A], z[A], wl.SMOOTH_LIMITS, *tA)
        try:
            st, _ = f.predict_core(th, locs[B], X[B], tB)
        finally:
            f.close()
        out.update(zip(B.tolist(), st.tolist()))
    return time.perf_counter() - t0, out


def time_taper_folds(g, delta, reps, refit_folds, counts=()):
    n = g * g
    locs, X, z, ref_taper = taper_problem(g, delta)
    th = wl.theta_full()
    labs = {"size10": size10_labels(n), "block100": fold_labels(locs, "block100"), "fold10": fold_labels(locs, "fold10")}
    if counts:                                  # --fold-counts: k random folds of n / k instead of the three cases
        labs = {"fold%d" % k: np.random.default_rng(7).permutation(n) % k for k in counts}
    out = {"n": n, "delta": delta, "nnz": int(ref_taper[0].size), "refit_folds_timed": refit_folds}
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
    resid = {}
    try:
        info = fit.krige_taper_info()
        out["W"], out["nt"] = info["W"], info["nt"]
        out["loo_ms"] = best(lambda: fit.cv_core(th), reps)
        for name, lab in labs.items():
            ts = []
            fit.cv_core(th, lab)
            for _ in range(reps):
                t0 = time.perf_counter()
                resid[name], _ = fit.cv_core(th, lab)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[name + "_ms"], out[name + "_runs_ms"] = min(ts), [round(t, 2) for t in ts]
            out[name + "_stats5"] = fit.last_cv_stats
            out[name + "_bytes"] = fit.last_cv_stats[4]
            print("n = %d %s: %.1f ms, stats5 %s" % (n, name, out[name + "_ms"], fit.last_cv_stats), file=sys.stderr, flush=True)
    finally:
        fit.close()
    R = z.reshape(n, -1)[:, 0] - X @ th["mean"]
    for name, lab in labs.items():
        nf = int(np.unique(lab).size)
        k = min(refit_folds, nf)
        secs, st = refit_taper(th, locs, X, z, ref_taper, lab, k)          # (the first fold's run warms the code paths up:
        secs, st = refit_taper(th, locs, X, z, ref_taper, lab, k)          # timed the second time)
        idx = np.array(sorted(st))
        out["refit_" + name + "_ms"] = secs * 1e3 * nf / k
        out["refit_" + name + "_scaled_from"] = [k, nf]
        out[name + "_vs_refit_max_abs"] = float(np.max(np.abs(resid[name][idx, 0] - (R[idx] - np.array([st[i] for i in idx])))))
        out[name + "_over_refit"] = out[name + "_ms"] / out["refit_" + name + "_ms"]
        print("n = %d %s: refit %.1f ms (from %d of %d folds), max |difference| %.2e" %
              (n, name, out["refit_" + name + "_ms"], k, nf, out[name + "_vs_refit_max_abs"]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--taper", action="store_true", help="leave-one-out on taper handles (cocons_cv_taper)")
    ap.add_argument("--taper-folds", action="store_true", help="folds on taper handles (cocons_cv_taper_folds)")
    ap.add_argument("--fold-counts", default="", help="--taper-folds with k random folds of equal size for these k, e.g. 15,20,40")
    ap.add_argument("--refit-folds", type=int, default=3, help="folds the refit route of --taper-folds is timed on (then scaled)")
    ap.add_argument("--taper-grids", default="100:0.06,316:0.019", help="g:delta pairs of the --taper / --taper-folds run")
    ap.add_argument("--stages-only", type=int, default=0, help="n: only cross-validation calls (for a rocprofv3 run)")
    ap.add_argument("--mode", choices=("loo", "fold10", "block100"), default="fold10")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    grids = [(int(s.split(":")[0]), float(s.split(":")[1])) for s in a.taper_grids.split(",")]
    if a.stages_only and a.taper_folds:
        locs, X, z, ref_taper = taper_problem(*grids[0])
        fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, *ref_taper)
        for _ in range(a.reps):
            fit.cv_core(wl.theta_full(), fold_labels(locs, a.mode))
        fit.close()
        return
    if a.stages_only:
        locs, X, z = problem(a.stages_only)
        fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
        for _ in range(a.reps):
            fit.cv_core(wl.theta_full(), fold_labels(locs, a.mode))
        fit.close()
        return
    if a.taper_folds:
        counts = tuple(int(k) for k in a.fold_counts.split(",") if k)
        res = {"taper_folds": [time_taper_folds(g, d, a.reps, a.refit_folds, counts) for g, d in grids]}
    elif a.taper:
        res = {"taper": [time_taper(g, d, a.reps) for g, d in grids]}
    else:
        res = {"sizes": [time_size(int(float(s)), a.reps) for s in a.sizes.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
