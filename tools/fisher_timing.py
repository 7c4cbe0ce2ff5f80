#!/usr/bin/env python3
"""Expected information of the dense model (cocons_fisher_dense): best-of-reps wall time of three second-order
routes on ONE handle in one run (C4 model, P = 16), at n = 4096 and n = 10^4:
  fisher    one host.getFisher_dense call (one factorisation, P products);
  hessian   host.getHessian_dense: 3 P (P + 1) / 2 = 408 batched objective values -- the route the project had;
  grad2P    2P = 32 calls of cocons_neg2loglik_grad_dense -- the cheapest second-order route a caller could assemble by hand.
Stage times of the Fisher call come from a run of `--stages-only N --reps K` under rocprofv3 --kernel-trace --stats -f csv,
summarised with `--stats-csv FILE --n N --calls K --ndir P`.
With --reml the same for the REML fit (cocons_fisher_reml), P = 16 without a free mean:
  fisher_reml    one host.getFisher_reml call;
  fisher_dense   one host.getFisher_dense call on the same handle;
  hessian_reml   the finite-difference REML Hessian: 3 P (P + 1) / 2 sequential GetNeg2loglikelihoodREML values (REML has no
                 batch entry);
and --stages-only runs getFisher_reml calls, whose summary adds the projector kernel beside the 16 n_pad^2 bytes it moves.
One JSON line.
usage: tools/fisher_timing.py [--reml] [--sizes 4096,10000] [--reps 5] [--stages-only N]
                              [--stats-csv FILE --n N --calls K --ndir P]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca  # noqa: E402
from cocons_amd import host, workloads as wl  # noqa: E402


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


def time_size(n, reps):
    locs, X, z = problem(n)
    pp = wl.par_pos_full()
    x0 = wl.theta_vector_from_lists(wl.theta_full(), pp)
    lam = (0.0, 0.0, 0.0)
    P = x0.size
    npad = (n + 127) // 128 * 128
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        tl = host.getModelLists(x0, pp, "diff")
        info = host.getFisher_dense(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, fit=fit)
        d = np.sqrt(np.diag(info))
        out = {"n": n, "P": int(P),
               "fisher_ms": best(lambda: host.getFisher_dense(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, fit=fit), reps),
               "hessian_ms": best(lambda: host.getHessian_dense(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit), reps),
               "grad2P_ms": best(lambda: [fit.neg2loglik_grad_core(tl) for _ in range(2 * P)], reps),
               "call_bytes": int(8 * ((P + 2) * npad * npad + P * P * (npad // 64) ** 2 + 6 * P * npad)),
               "min_eig_normalised": float(np.linalg.eigvalsh(info / np.outer(d, d))[0])}
    finally:
        fit.close()
    out["fisher_over_hessian"] = out["fisher_ms"] / out["hessian_ms"]
    out["fisher_over_grad2P"] = out["fisher_ms"] / out["grad2P_ms"]
    return out


def reml_start():
    """(par_pos, x0) of the C4 model; par_pos_full has no free mean entry, as cocoOptim's reml branch requires"""
    pp = wl.par_pos_full()
    return pp, wl.theta_vector_from_lists(wl.theta_full(), pp)


def reml_hessian(x0, pp, locs, X, z, n, lam, fit, eps=np.finfo(float).eps ** 0.25):
    """getHessian_dense's scheme on GetNeg2loglikelihoodREML, one value after the other"""
    def f(x):
        return host.GetNeg2loglikelihoodREML(x, pp, locs, X, None, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)
    P = x0.size
    f00 = f(x0)
    H = np.zeros((P, P))
    for jj in range(P):
        for ii in range(jj, P):
            t01, t10, t11 = x0.copy(), x0.copy(), x0.copy()
            t01[jj] += eps
            t10[ii] += eps
            t11[jj] += eps
            t11[ii] += eps
            H[jj, ii] = 0.5 * ((f(t11) - f(t01) - f(t10) + f00) / (eps * eps))
    H = H + H.T
    H[np.diag_indices(P)] /= 2
    return H


def time_size_reml(n, reps):
    locs, X, z = problem(n)
    pp, x0 = reml_start()
    lam = (0.0, 0.0, 0.0)
    P = x0.size
    npad = (n + 127) // 128 * 128
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        info = host.getFisher_reml(x0, pp, locs, X, None, wl.SMOOTH_LIMITS, z, n, fit=fit)
        d = np.sqrt(np.diag(info))
        out = {"n": n, "P": int(P),
               "fisher_reml_ms": best(lambda: host.getFisher_reml(x0, pp, locs, X, None, wl.SMOOTH_LIMITS, z, n, fit=fit), reps),
               "fisher_dense_ms": best(lambda: host.getFisher_dense(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, fit=fit), reps),
               "hessian_reml_ms": best(lambda: reml_hessian(x0, pp, locs, X, z, n, lam, fit), reps),
               "hessian_reml_values": 3 * P * (P + 1) // 2 + 1,
               "projector_bytes": int(16 * npad * npad),
               "min_eig_normalised": float(np.linalg.eigvalsh(info / np.outer(d, d))[0])}
    finally:
        fit.close()
    out["reml_over_hessian"] = out["fisher_reml_ms"] / out["hessian_reml_ms"]
    out["reml_over_dense"] = out["fisher_reml_ms"] / out["fisher_dense_ms"]
    return out


def stages(csv_path, n, calls, ndir):
    """Per-call device time of the Fisher call's stages from the kernel stats of a --stages-only run.  The factorisation, its
    L^-T border, -L^-T L^-1 and the ndir products all run the trailing-update kernel: one stage, 5/3 n^3 + 2 ndir n^3 flops."""
    tot = {}
    for r in csv.DictReader(open(csv_path)):
        name = r.get("Name") or r.get("KernelName") or ""
        tot[name] = tot.get(name, 0.0) + float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)

    def ms(*keys):
        return sum(v for k, v in tot.items() if any(key in k for key in keys)) / calls * 1e-6

    npad = (n + 127) // 128 * 128
    st = {"trailing_updates_ms": ms("update_kernel"),
          "panels_ms": ms("panel_pair_kernel", "potrf_tile", "trsm_tile", "potrf_follow"),
          "assembly_ms": ms("pair_sym_kernel", "loc_params_kernel", "rhs_rows_kernel", "grad_fill_kernel"),
          "directions_ms": ms("dsigma_dirs_kernel", "fisher_weight_kernel", "grad_site_kernel"),
          "mirror_ms": ms("fisher_mirror_kernel"),
          "trace_ms": ms("fisher_trace"),
          "mean_block_ms": ms("fisher_sx_kernel", "fisher_xtsx_kernel", "grad_sigma_r")}
    flops = (5.0 / 3.0 + 2.0 * ndir) * float(npad) ** 3
    st["trailing_tflops"] = flops / (st["trailing_updates_ms"] * 1e-3) / 1e12
    if any("fisher_project_kernel" in k for k in tot):       # (a --reml run)
        st["projector_ms"] = ms("fisher_project_kernel")
        st["projector_bytes"] = 16 * npad * npad
        st["projector_tb_per_s"] = st["projector_bytes"] / (st["projector_ms"] * 1e-3) / 1e12
        st["lowrank_ms"] = ms("grad_gls_kernel", "grad_lowrank_kernel")
    return {"n": n, "calls": calls, "ndir": ndir, "per_call": st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reml", action="store_true", help="the REML fit's information (cocons_fisher_reml)")
    ap.add_argument("--stages-only", type=int, default=0, help="n: only Fisher calls (for a rocprofv3 run)")
    ap.add_argument("--stats-csv", default="")
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=3, help="Fisher calls of the --stages-only run the stats cover")
    ap.add_argument("--ndir", type=int, default=16)
    a = ap.parse_args()
    if a.stats_csv:
        print(json.dumps(stages(a.stats_csv, a.n, a.calls, a.ndir)))
        return
    if a.stages_only:
        n = a.stages_only
        locs, X, z = problem(n)
        pp = wl.par_pos_full()
        x0 = wl.theta_vector_from_lists(wl.theta_full(), pp)
        if a.reml:
            pp, x0 = reml_start()
        fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
        for _ in range(a.reps):          # (profile with --reps equal to --calls of the summary)
            if a.reml:
                host.getFisher_reml(x0, pp, locs, X, None, wl.SMOOTH_LIMITS, z, n, fit=fit)
            else:
                host.getFisher_dense(x0, pp, locs, X, wl.SMOOTH_LIMITS, z, n, fit=fit)
        fit.close()
        return
    one = time_size_reml if a.reml else time_size
    print(json.dumps({"sizes": [one(int(float(s)), a.reps) for s in a.sizes.split(",")]}))


if __name__ == "__main__":
    main()
