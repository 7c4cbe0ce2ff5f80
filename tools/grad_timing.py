#!/usr/bin/env python3
"""Analytic gradient of the dense -2 log-likelihood (cocons_neg2loglik_grad_dense): wall time of one value + gradient call
against one cocons_neg2loglik_dense and against the 1 + 2P = 33-point cocons_neg2loglik_batch of a central-difference
gradient (C4 model, P = 16), at n = 4096 and n = 10^4; and an L-BFGS-B run (scipy) from the C4 start at n = 4096 with the
analytic gradient against the central-difference gradient through the batch: iterations, end value, wall time.
Stage times come from a run of `--stages-only N --reps K` under rocprofv3 --kernel-trace --stats -f csv, summarised with
`--stats-csv FILE --n N --calls K`: the trailing updates (factorisation, L^-T border and the product -L^-T L^-1 share one
kernel and are reported together, at their executed and their useful TFLOP/s), panels, assembly, Sigma^-1 R, contraction.
--objective pml | reml does the same for cocons_neg2loglik_profile_grad / _reml_grad (x_betas = X, the mean profiled out):
one value call, one value + gradient call, the 1 + 2P sequential value calls of a central difference, the dense gradient call
on the same handle, and the L-BFGS-B comparison with and without the analytic gradient.
One JSON line.
usage: tools/grad_timing.py [--objective ml|pml|reml] [--sizes 4096,10000] [--reps 5] [--no-optim] [--stages-only N] [--stats-csv FILE --n N --calls K]"""
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


def fd_points(x, h):
    pts = [x.copy()]
    for i in range(x.size):
        for s in (h, -h):
            y = x.copy()
            y[i] += s
            pts.append(y)
    return pts


def time_size(n, reps):
    locs, X, z = problem(n)
    th = wl.theta_full()
    pp = wl.par_pos_full()
    x0 = wl.theta_vector_from_lists(th, pp)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    try:
        tl = host.getModelLists(x0, pp, "diff")
        tls = [host.getModelLists(y, pp, "diff") for y in fd_points(x0, 1.2e-4)]
        out = {"n": n,
               "value_ms": best(lambda: fit.neg2loglik_core(tl), reps),
               "grad_ms": best(lambda: fit.neg2loglik_grad_core(tl), reps),
               "batch33_ms": best(lambda: fit.neg2loglik_batch_core(tls), max(1, reps // 2))}
    finally:
        fit.close()
    out["grad_over_value"] = out["grad_ms"] / out["value_ms"]
    out["grad_over_batch33"] = out["grad_ms"] / out["batch33_ms"]
    return out


def optim(n, maxiter):
    from scipy.optimize import minimize
    locs, X, z = problem(n)
    pp = wl.par_pos_full()
    x0 = wl.theta_vector_from_lists(wl.theta_full(), pp)
    lam = (0.0, 0.0, 0.0)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    res = {}
    try:
        def fg(x):
            return host.GetNeg2loglikelihood_grad(x, pp, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)

        def fg_fd(x, h=1.2e-4):
            v = host.GetNeg2loglikelihood_batch(fd_points(x, h), pp, locs, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)
            return v[0], (v[1::2] - v[2::2]) / (2 * h)

        for name, fun in (("analytic", fg), ("central_difference", fg_fd)):
            t0 = time.perf_counter()
            r = minimize(fun, x0, jac=True, method="L-BFGS-B", options={"maxiter": maxiter})
            res[name] = {"iterations": int(r.nit), "evaluations": int(r.nfev), "value": float(r.fun),
                         "wall_s": time.perf_counter() - t0, "message": str(r.message)}
    finally:
        fit.close()
    return res


def _profiled(objective, locs, X, z, n):
    """(fit, par_pos, x0, value(x), value_and_gradient(x), core value call, core gradient call) of --objective pml | reml:
    x_betas = X (q = p = 3), the mean profiled out (par_pos["mean"] all False)."""
    pp = wl.par_pos_full()
    pp["mean"] = [False] * X.shape[1]
    x0 = wl.theta_vector_from_lists(wl.theta_full(), pp)
    lam = (0.0, 0.0, 0.0)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS, x_betas=X)
    rank = int(np.linalg.matrix_rank(X))
    if objective == "pml":
        def value(x):
            return host.GetNeg2loglikelihoodProfile(x, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=fit)

        def fg(x):
            return host.GetNeg2loglikelihoodProfile_grad(x, pp, locs, X, wl.SMOOTH_LIMITS, z, n, X, lam, fit=fit)
        core, core_grad = fit.neg2loglik_profile_core, fit.neg2loglik_profile_grad_core
    else:
        def value(x):
            return host.GetNeg2loglikelihoodREML(x, pp, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)

        def fg(x):
            return host.GetNeg2loglikelihoodREML_grad(x, pp, locs, X, X, wl.SMOOTH_LIMITS, z, n, lam, fit=fit)

        def core(tl):
            return fit.neg2loglik_reml_core(tl, rank)

        def core_grad(tl):
            return fit.neg2loglik_reml_grad_core(tl, rank)
    return fit, pp, x0, value, fg, core, core_grad


def time_size_profiled(objective, n, reps):
    """One value call, one value + gradient call, the 1 + 2P SEQUENTIAL value calls of a central difference (there is no
    batch entry for these objectives), and the dense gradient call on the same handle for comparison."""
    locs, X, z = problem(n)
    fit, pp, x0, value, fg, core, core_grad = _profiled(objective, locs, X, z, n)
    try:
        tl = host.getModelLists(x0, pp, "diff")
        tls = [host.getModelLists(y, pp, "diff") for y in fd_points(x0, 1.2e-4)]
        out = {"n": n, "objective": objective, "points": len(tls),
               "value_ms": best(lambda: core(tl), reps),
               "grad_ms": best(lambda: core_grad(tl), reps),
               "sequential_ms": best(lambda: [core(t) for t in tls], max(1, reps // 2)),
               "dense_grad_ms": best(lambda: fit.neg2loglik_grad_core(tl), reps)}
    finally:
        fit.close()
    out["grad_over_value"] = out["grad_ms"] / out["value_ms"]
    out["grad_over_sequential"] = out["grad_ms"] / out["sequential_ms"]
    return out


def optim_profiled(objective, n, maxiter):
    from scipy.optimize import minimize
    locs, X, z = problem(n)
    fit, pp, x0, value, fg, core, core_grad = _profiled(objective, locs, X, z, n)
    res = {}
    try:
        def fg_fd(x, h=1.2e-4):
            v = np.array([value(y) for y in fd_points(x, h)])
            return v[0], (v[1::2] - v[2::2]) / (2 * h)

        for name, fun in (("analytic", fg), ("central_difference", fg_fd)):
            t0 = time.perf_counter()
            r = minimize(fun, x0, jac=True, method="L-BFGS-B", options={"maxiter": maxiter})
            res[name] = {"iterations": int(r.nit), "evaluations": int(r.nfev), "value": float(r.fun),
                         "wall_s": time.perf_counter() - t0, "message": str(r.message)}
    finally:
        fit.close()
    return res


PEAK_F64_MFMA = 78.6e12    # TFLOP/s of v_mfma_f64_16x16x4_f64 over the chip


def stages(csv_path, n, calls):
    """Per-call device time of every stage from the kernel stats of a --stages-only run (`calls` gradient calls), and the
    rate of the trailing updates.  The factorisation, the L^-T border and the product -B B' all run the same trailing-update
    kernel, so they are ONE stage here.  Its work: n^3 / 3 (factorisation) + about n^3 (border rows updated as full
    rectangles) + n^3 / 3 (product) = 5/3 n^3 executed, of which n^3 is useful (the border's updates of L^-T's zero lower
    triangle are not): both rates are reported."""
    tot = {}
    for r in csv.DictReader(open(csv_path)):
        name = r.get("Name") or r.get("KernelName") or ""
        ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
        tot[name] = tot.get(name, 0.0) + ns

    def ms(*keys):
        return sum(v for k, v in tot.items() if any(key in k for key in keys)) / calls * 1e-6

    npad = (n + 127) // 128 * 128
    st = {"trailing_updates_ms": ms("update_kernel"),
          "panels_ms": ms("panel_pair_kernel", "potrf_tile", "trsm_tile", "potrf_follow"),
          "assembly_ms": ms("pair_sym_kernel", "loc_params_kernel", "rhs_rows_kernel", "grad_fill_kernel"),
          "sigma_r_ms": ms("grad_sigma_r"),
          "contraction_ms": ms("grad_pair_kernel", "grad_reduce_kernel", "grad_xt_kernel", "grad_site_kernel"),
          "reductions_ms": ms("finalize_kernel")}
    t = st["trailing_updates_ms"] * 1e-3
    executed, useful = 5.0 / 3.0 * npad ** 3, float(npad) ** 3
    st["trailing_tflops_executed"] = executed / t / 1e12
    st["trailing_tflops_useful"] = useful / t / 1e12
    st["trailing_frac_executed"] = executed / t / PEAK_F64_MFMA
    st["trailing_frac_useful"] = useful / t / PEAK_F64_MFMA
    return {"n": n, "calls": calls, "per_call": st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-optim", action="store_true")
    ap.add_argument("--maxiter", type=int, default=60)
    ap.add_argument("--stages-only", type=int, default=0, help="n: only gradient calls (for a rocprofv3 run)")
    ap.add_argument("--stats-csv", default="")
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=3, help="gradient calls of the --stages-only run the stats cover")
    ap.add_argument("--objective", choices=("ml", "pml", "reml"), default="ml",
                    help="pml / reml: the Profile / REML value and gradient entries against 1 + 2P sequential value calls")
    a = ap.parse_args()
    if a.stats_csv:
        print(json.dumps(stages(a.stats_csv, a.n, a.calls)))
        return
    if a.objective != "ml":
        if a.stages_only:
            locs, X, z = problem(a.stages_only)
            fit, pp, x0, value, fg, core, core_grad = _profiled(a.objective, locs, X, z, a.stages_only)
            tl = host.getModelLists(x0, pp, "diff")
            for _ in range(a.reps):
                core_grad(tl)
            fit.close()
            return
        out = {"objective": a.objective,
               "sizes": [time_size_profiled(a.objective, int(float(s)), a.reps) for s in a.sizes.split(",")]}
        if not a.no_optim:
            out["lbfgsb_n4096"] = optim_profiled(a.objective, 4096, a.maxiter)
        print(json.dumps(out))
        return
    if a.stages_only:
        locs, X, z = problem(a.stages_only)
        fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
        th = wl.theta_full()
        for _ in range(a.reps):          # (profile with --reps equal to --calls of the summary)
            fit.neg2loglik_grad_core(th)
        fit.close()
        return
    out = {"sizes": [time_size(int(float(s)), a.reps) for s in a.sizes.split(",")]}
    if not a.no_optim:
        out["lbfgsb_n4096"] = optim(4096, a.maxiter)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
