#!/usr/bin/env python3
"""Expected information of a tapered fit (cocons_fisher_taper): best-of-reps wall time of four second-order
routes on ONE taper handle in one run, on the g x g grid and taper range of tools/taper_timing.py (100 / 0.06, 316 / 0.019)
with the 13 free parameters of DESIGN.md 4i (std.dev, scale, smooth over three columns, the nugget intercept, the mean):
  probed   (a) one cocons_fisher_taper call with 64 random +-1 probes (10 covariance directions; the mean block is exact);
  exact    (b) one call in exact mode (--exact-once: a single timed call, for n = 99 856; --no-exact: none);
  batch    (c) 1 + 3 P (P + 1) / 2 = 274 objective values through cocons_neg2loglik_batch: the route a caller had;
  grad2P   (d) 2 P = 26 calls of cocons_neg2loglik_grad_taper.
With an exact result at hand the metric max |I - R| / sqrt(R_aa R_bb) of (a) against (b) is recorded for seeds 0 .. 4.
One JSON line, also written to profiles/fisher_taper_timing_n<n>.json.  --calls K [--trace-exact]: only K probed calls (and
one exact call) after a warm-up, for a run under rocprofv3 --kernel-trace --stats; --stats-csv FILE --calls K sums such a
run's kernel stats per stage.
usage: tools/fisher_taper_timing.py [g=100] [delta=0.06] [--reps 5] [--exact-once | --no-exact] [--calls K [--trace-exact]]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = (("sweep_diag", ("krige_band_diag",)),
          ("sweep_update", ("krige_band_update",)),
          ("pack", ("krige_band_pack", "krige_band_qprep", "band_back_pack", "band_back_qprep")),
          ("directions", ("taper_dirs", "grad_site")),
          ("factor", ("potrf", "trsm", "update_kernel", "taper_kernel", "band_zero", "pad_identity", "loc_params", "rhs_rows", "follow")),
          ("spmm", ("band_spmm_dirs",)),
          ("gram", ("band_gram",)),
          ("rows", ("band_unit_rows", "band_given_rows", "band_x_rows")))


def stages(csv_path, calls):
    tot, cnt = {}, {}
    for r in csv.DictReader(open(csv_path)):
        name = r.get("Name") or r.get("KernelName") or ""
        tot[name] = tot.get(name, 0.0) + float(r.get("TotalDurationNs") or 0)
        cnt[name] = cnt.get(name, 0) + int(float(r.get("Calls") or 0))
    out, seen = {}, set()
    for st, keys in STAGES:
        names = [k for k in tot if any(key in k for key in keys) and k not in seen]
        seen.update(names)
        out[st + "_ms"] = sum(tot[k] for k in names) / calls * 1e-6
        out[st + "_launches"] = sum(cnt[k] for k in names) / calls
    out["other_ms"] = sum(v for k, v in tot.items() if k not in seen) / calls * 1e-6
    return {"calls": calls, "per_call": out}


def pattern(locs, delta):
    """Wendland-1 taper of range delta (1-based CSR), by cells of edge delta"""
    ci, rp, ent, cell = [], [1], [], {}
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
    return np.array(ci, dtype=np.int32), np.array(rp, dtype=np.int32), np.array(ent)


def metric(I, R):
    d = np.sqrt(np.where(np.diag(R) == 0, 1.0, np.diag(R)))
    return float(np.max(np.abs(I - R) / np.outer(d, d)))


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("g", nargs="?", type=int, default=100)
    ap.add_argument("delta", nargs="?", type=float, default=0.06)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--exact-once", action="store_true")
    ap.add_argument("--no-exact", action="store_true")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--trace-exact", action="store_true")
    ap.add_argument("--stats-csv", default="")
    a = ap.parse_args()
    if a.stats_csv:
        print(json.dumps(stages(a.stats_csv, max(a.calls, 1))))
        return
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    g, delta = a.g, a.delta
    n = g * g
    locs = wl.grid_locs(g)
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full()
    z = wl.synthetic_z(n)
    t0 = time.perf_counter()
    ci, rp, ent = pattern(locs, delta)
    print("pattern: n = %d, nnz = %d (%.1f per row), built in %.1f s" % (n, ci.size, ci.size / n, time.perf_counter() - t0), flush=True)
    fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, ci, rp, ent)
    names = [(k, i) for k in ("std.dev", "scale", "smooth") for i in range(3)] + [("nugget", 0)] + [("mean", i) for i in range(3)]
    P = len(names)
    rows_of = {"std.dev": 0, "scale": 1, "smooth": 4, "nugget": 5}
    dirs = np.zeros((10, 6, 3))
    for a_, (k, i) in enumerate(names[:10]):
        dirs[a_, rows_of[k], i] = 1.0

    def probes(seed):
        return np.random.default_rng(seed).integers(0, 2, size=(n, a.nprobe)) * 2.0 - 1.0

    P0 = probes(0)
    info = fit.krige_taper_info()
    out = {"n": n, "delta": delta, "nnz": int(ci.size), "P": P, "ndir": 10, "nprobe": a.nprobe, "W": info["W"], "nt": info["nt"]}
    fit.neg2loglik_core(th)
    if a.calls:
        fit.fisher_core(th, dirs, probes=P0)
        for _ in range(a.calls):
            fit.fisher_core(th, dirs, probes=P0)
        if a.trace_exact:
            fit.fisher_core(th, dirs)
        fit.close()
        return

    def shifted(steps):
        t2 = {kk: np.array(vv, dtype=float) for kk, vv in th.items()}
        for (k, i), s_ in steps:
            t2[k][i] += s_
        return t2
    eps = np.finfo(float).eps ** 0.25
    pts = [th]
    for jj in range(P):
        for ii in range(jj, P):
            pts += [shifted([(names[jj], eps)]), shifted([(names[ii], eps)]), shifted([(names[jj], eps), (names[ii], eps)])]
    assert len(pts) == 1 + 3 * P * (P + 1) // 2
    out["batch_points"] = len(pts)
    out["value_ms"] = best(lambda: fit.neg2loglik_core(th), a.reps)
    out["probed_ms"] = best(lambda: fit.fisher_core(th, dirs, probes=P0), a.reps)
    print("probed: %.1f ms" % out["probed_ms"], flush=True)
    out["grad2P_ms"] = best(lambda: [fit.neg2loglik_grad_core(th) for _ in range(2 * P)], a.reps)
    print("grad2P: %.1f ms" % out["grad2P_ms"], flush=True)
    fit.neg2loglik_batch_core(pts[:4])
    out["batch_ms"] = best(lambda: fit.neg2loglik_batch_core(pts), a.reps)
    print("batch: %.1f ms" % out["batch_ms"], flush=True)
    exact = None
    if not a.no_exact:
        if a.exact_once:
            t0 = time.perf_counter()
            exact = fit.fisher_core(th, dirs)
            out["exact_ms"] = (time.perf_counter() - t0) * 1e3
            out["exact_calls_timed"] = 1
        else:
            out["exact_ms"] = best(lambda: fit.fisher_core(th, dirs), a.reps)
            exact = fit.fisher_core(th, dirs)
        print("exact: %.1f ms" % out["exact_ms"], flush=True)
        out["probed_vs_exact_seeds_0_4"] = [metric(fit.fisher_core(th, dirs, probes=probes(s))[0], exact[0]) for s in range(5)]
        est = fit.fisher_core(th, dirs, probes=P0)
        out["info_mean_probed_equals_exact"] = bool(np.array_equal(est[1], exact[1]))
        dd = np.sqrt(np.diag(exact[0]))
        out["min_eig_normalised"] = float(np.linalg.eigvalsh(exact[0] / np.outer(dd, dd))[0])
        out["exact_over_batch"] = out["exact_ms"] / out["batch_ms"]
    out["probed_over_batch"] = out["probed_ms"] / out["batch_ms"]
    out["probed_over_grad2P"] = out["probed_ms"] / out["grad2P_ms"]
    fit.close()
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fisher_taper_timing_n%d.json" % n), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
