"""Time the taper objective (GetNeg2loglikelihoodTaper through the band-limited dense-tile factorisation on the device)
on a g x g grid with a Wendland-1 taper of range delta: python tools/taper_timing.py [g=100] [delta=0.06] [cpu].
The CPU comparison (SuperLU) runs for n <= 12000 or when the third argument is "cpu" (300 s at n = 40000).

--grad: time cocons_neg2loglik_grad_taper instead -- one value + gradient call against cocons_neg2loglik_batch over the
1 + 2P points of a central-difference gradient of the same model (P = 13: std.dev, scale, smooth over three columns, the
nugget intercept, the mean) on the same handle in the same run, and against one value call; the lines go to
profiles/grad_taper_timing_n<n>.txt as well.  --lbfgs (with --grad): L-BFGS-B on the taper objective from one start with the
analytic gradient and with batched central differences, the same number of iterations, end values side by side.
--calls K (with --grad): only K gradient calls after one warm-up (for a kernel trace)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cocons_amd as ca                     # noqa: E402
from cocons_amd import workloads as wl     # noqa: E402

FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
CALLS = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
sys.argv = [a for i, a in enumerate(sys.argv) if not a.startswith("--") and not (i > 0 and sys.argv[i - 1] == "--calls")]
g = int(sys.argv[1]) if len(sys.argv) > 1 else 100
delta = float(sys.argv[2]) if len(sys.argv) > 2 else 0.06
n = g * g
locs = wl.grid_locs(g)
X = wl.design_from_locs(locs)["std.covs"]
th = wl.theta_full()
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
print("pattern: n = %d, nnz = %d (%.1f per row, %.2f %% dense), built in %.1f s" %
      (n, len(ci), len(ci) / n, 100.0 * len(ci) / n / n, time.perf_counter() - t0))


def device_free_bytes():
    """free device memory (hipMemGetInfo through ctypes): the handle's footprint is the drop across its creation"""
    import ctypes
    from cocons_amd.shard import _hip_runtime
    hip = _hip_runtime()
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    return free.value


ca.CoconsFit(locs[:300], X[:300], z[:300], wl.SMOOTH_LIMITS).neg2loglik_core(th)   # library + context are up
free0 = device_free_bytes()
fit = ca.CoconsTaperFit(locs, X, z, wl.SMOOTH_LIMITS, np.array(ci, dtype=np.int32), np.array(rp, dtype=np.int32), np.array(ent))
for _ in range(3):
    v, parts = fit.neg2loglik_core(th)
print("device memory of the handle (pattern, data, factorisation buffer): %.3f GB; a dense n x n buffer alone: %.2f GB" %
      ((free0 - device_free_bytes()) / 1e9, 8.0 * n * n / 1e9))


def grad_report():
    """one value + gradient call against the batch over the 1 + 2P central-difference points and against one value call"""
    lines = ["python tools/taper_timing.py %d %g --grad%s" % (g, delta, " --lbfgs" if "--lbfgs" in FLAGS else ""),
             "n = %d, delta = %g, nnz = %d, r = 1" % (n, delta, len(ci))]
    names = [(k, i) for k in ("std.dev", "scale", "smooth") for i in range(3)] + [("nugget", 0)] + [("mean", i) for i in range(3)]
    P = len(names)

    def shifted(k, i, step):
        t2 = {kk: np.array(vv, dtype=float) for kk, vv in th.items()}
        t2[k][i] += step
        return t2
    h = 1e-4
    pts = [th] + [shifted(k, i, s_ * h) for k, i in names for s_ in (1, -1)]
    fit.neg2loglik_grad_core(th)
    fit.neg2loglik_batch_core(pts[:4])
    if CALLS:
        for _ in range(CALLS):
            fit.neg2loglik_grad_core(th)
        return
    reps = 5
    tv, tg, tb = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fit.neg2loglik_core(th); tv.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); val, parts, gt, gq, gm = fit.neg2loglik_grad_core(th); tg.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); vals, st = fit.neg2loglik_batch_core(pts); tb.append(time.perf_counter() - t0)
    tv, tg, tb = min(tv), min(tg), min(tb)
    rows_of = {"std.dev": 0, "scale": 1, "smooth": 4, "nugget": 5}
    ana = np.array([gm[i] if k == "mean" else gt[rows_of[k], i] for k, i in names])
    num = (vals[1::2] - vals[2::2]) / (2 * h)
    lines.append("one value call: %.2f ms; one value + gradient call: %.2f ms (%.2f value calls)" % (1e3 * tv, 1e3 * tg, tg / tv))
    lines.append("batch over the 1 + 2P = %d points (P = %d): %.2f ms; gradient call / batch = %.3f" % (len(pts), P, 1e3 * tb, tg / tb))
    lines.append("analytic against the batch's central differences (all points ok: %s): max |diff| %.3e of %.3e" %
                 (bool(np.all(st == 0)), float(np.max(np.abs(ana - num))), float(np.max(np.abs(num)))))
    lines.append("scaling identity d/dsd0 + d/dnugget0 - (r n - sum of quadratic forms): %.3e of r n = %d" %
                 (abs(gt[0, 0] + gt[5, 0] - (n - float(np.sum(parts[1:])))), n))
    if os.environ.get("COCONS_TIMING_VERBOSE"):
        print("analytic", ana, "\nnumeric", num, "\nstatus", st, "\nvalues", vals, "\nvalue", val, parts)
    if "--lbfgs" in FLAGS:
        from scipy.optimize import minimize
        x0 = np.array([th[k][i] for k, i in names])

        def unpack(x):
            t2 = {kk: np.array(vv, dtype=float) for kk, vv in th.items()}
            for (k, i), xv in zip(names, x):
                t2[k][i] = xv
            return t2

        def f_ana(x):
            try:
                val, _, gt, _, gm = fit.neg2loglik_grad_core(unpack(x))
            except ca.CholeskyError:
                return 1e6, np.zeros(P)
            return val, np.array([gm[i] if k == "mean" else gt[rows_of[k], i] for k, i in names])

        def f_num(x):
            pp = [unpack(x)]
            for j in range(P):
                for s_ in (1, -1):
                    xx = x.copy(); xx[j] += s_ * h
                    pp.append(unpack(xx))
            vals, st = fit.neg2loglik_batch_core(pp)
            vals = np.where(st == 0, vals, 1e6)
            return vals[0], (vals[1::2] - vals[2::2]) / (2 * h)
        x0 = x0 + 0.1 * np.cos(np.arange(P))                 # a start off the generating parameters
        iters = 15
        out = {}
        for name, fun in (("analytic gradient", f_ana), ("batched differences", f_num)):
            t0 = time.perf_counter()
            res = minimize(fun, x0, jac=True, method="L-BFGS-B", options=dict(maxiter=iters, maxfun=10 * iters))
            out[name] = (time.perf_counter() - t0, res)
            lines.append("L-BFGS-B, %s: %d iterations, %d evaluations, %.2f s, end value %.6f" %
                         (name, res.nit, res.nfev, out[name][0], res.fun))
        lines.append("L-BFGS-B run time, batched differences / analytic gradient: %.2f" %
                     (out["batched differences"][0] / out["analytic gradient"][0]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"), exist_ok=True)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                           "grad_taper_timing_n%d.txt" % n), "w") as fh:
        fh.write(text + "\n")


if "--grad" in FLAGS:
    grad_report()
    sys.exit(0)
K = 20
t0 = time.perf_counter()
for _ in range(K):
    v, parts = fit.neg2loglik_core(th)
dt = (time.perf_counter() - t0) / K
print("taper objective: %.3f ms per evaluation (%.1f evals/s), value %.6f" % (1e3 * dt, 1 / dt, v))
nb = 33                                           # one finite-difference gradient of a 16-parameter model
tls = []
for i in range(nb):
    t2 = {k: np.array(v, dtype=float) for k, v in th.items()}
    t2["std.dev"][0] += 1e-3 * i
    tls.append(t2)
fit.neg2loglik_batch_core(tls[:4])
t0 = time.perf_counter()
vals, st = fit.neg2loglik_batch_core(tls)
dtb = time.perf_counter() - t0
print("batch of %d independent evaluations: %.1f evals/s (all ok: %s)" % (nb, nb / dtb, bool(np.all(st == 0))))
# context: a sparse direct factorisation of the same matrix on this host's CPU (scipy / SuperLU, one thread's worth of
# work; spam's supernodal Cholesky is not available here and would be roughly 2x cheaper than an LU)
if n > 12000 and not (len(sys.argv) > 3 and sys.argv[3] == "cpu") or (len(sys.argv) > 3 and sys.argv[3] == "nocpu"):
    sys.exit(0)
try:
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    vals = np.array(ent) * ca.cov_rns_taper(th, locs, X, np.array(ci, dtype=np.int32), np.array(rp, dtype=np.int32), wl.SMOOTH_LIMITS)
    S = sp.csr_matrix((vals, np.array(ci) - 1, np.array(rp) - 1), shape=(n, n)).tocsc()
    t0 = time.perf_counter()
    lu = spl.splu(S, permc_spec="MMD_AT_PLUS_A", options=dict(SymmetricMode=True))
    resid = z[:, 0] - X @ th["mean"] if z.ndim == 2 else z - X @ th["mean"]
    q = float(resid @ lu.solve(resid))
    dtc = time.perf_counter() - t0
    ld = float(np.sum(np.log(np.abs(lu.U.diagonal()))))
    vc = n * np.log(2 * np.pi) + ld + q
    print("CPU sparse LU of the same matrix: %.1f ms; value %.6f (rel. diff %.1e)" % (1e3 * dtc, vc, abs(vc - v) / abs(v)))
except Exception as e:          # noqa: BLE001
    print("CPU sparse comparison skipped:", e)
