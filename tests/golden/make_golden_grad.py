#!/usr/bin/env python3
"""Generate exact-arithmetic golden vectors for the analytic gradients (mpmath, 70 digits).

Nothing of the pair-partial algebra of grad.hip / tests/grad_reference.py is restated here: every gradient below is a
central difference (step 1e-24, 70 digits: truncation and rounding both below 1e-40 of the value) of the whole objective,
evaluated from the model of make_golden.py with the perturbation kept in mpmath from end to end.  Rounding happens once,
at the final float().

Outputs (small JSON, committed):
  matern_partials_grid.json   M = 2^(1-nu)/Gamma(nu) u^nu K_nu(u), dM/du = -2^(1-nu)/Gamma(nu) u^nu K_{nu-1}(u), dM/dnu and
                              the exact truncation of the four-point stencil (step 1e-3 nu) grad.hip takes for dM/dnu
  grad_dense_<case>.json      dense, Profile and REML objectives (tests/grad_profile_reference.py's definitions): value,
                              parts, d/d(6 x p table), d/dmean, cond(Sigma); the cases are listed in CASES
  grad_taper_n150.json        the tapered objective of tests/grad_taper_reference.py on wendland1_pattern(locs, 0.25):
                              value, parts, gradient split into its log-determinant and quadratic-form shares, d/dmean

Usage: python tests/golden/make_golden_grad.py            everything, then the ref_err blocks
       python tests/golden/make_golden_grad.py --ref-err  only (re)fill the ref_err block of every fixture: the error of the
                                                          float64 statements tests/grad*_reference.py against the golden,
                                                          per family -- the measurement the GPU tests' bounds rest on
       python tests/golden/make_golden_grad.py --only grid|taper|<case> ...
Run by hand, never at test time.  About 15 minutes on 8 cores.
"""
import json
import math
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402

DPS = 70
mp.mp.dps = DPS
STEP_EXP = -24
ROWS = ("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
TAPER_ROWS = ("std.dev", "scale", "smooth", "nugget")
TAPER_DELTA = 0.25
WORKERS = min(16, os.cpu_count() or 1)

GRID_NU = [0.01, 0.05, 0.1, 0.25, 0.4, 0.45, 0.499999, 0.5, 0.500001, 0.75, 0.999999, 1.0, 1.000001, 1 + 1e-9, 1.3, 1.5, 2.0,
           2.4999, 2.5, 3.0, 3.5, 3.500001, 5.7, 8.0, 12.0, 15.0]
GRID_U = [1e-10, 1e-8, 1e-6, 1e-4, 1e-3, 1e-2, 0.1, 0.5, 1.0, 1.9999999, 2.0, 2.0000001, 3.0, 5.0, 8.0, 13.0, 19.99, 20.0,
          20.01, 60.0, 150.0, 400.0, 700.0, 705.99]


def fl(x):
    return float(x)


def step():
    return mp.mpf(10) ** STEP_EXP


# --------------------------------------------------------------------------- #
# Matern partials on a grid
# --------------------------------------------------------------------------- #
def matern(nu, u):
    return mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(u, nu) * mp.besselk(nu, u)


def grid_row(args):
    nu_f, u_f = args
    mp.mp.dps = DPS
    nu, u = mp.mpf(nu_f), mp.mpf(u_f)
    M = matern(nu, u)
    Mu = -mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(u, nu) * mp.besselk(nu - 1, u)
    d = step()
    Mn = (matern(nu + d, u) - matern(nu - d, u)) / (2 * d)
    h = mp.mpf(1e-3) * nu                  # the double 1e-3, as the device multiplies it
    S = (8 * (matern(nu + h, u) - matern(nu - h, u)) - (matern(nu + 2 * h, u) - matern(nu - 2 * h, u))) / (12 * h)
    return {"nu": nu_f, "u": u_f, "M": fl(M), "dM_du": fl(Mu), "dM_dnu": fl(Mn), "dnu_trunc": fl(abs(S - Mn))}


def write_grid(rows):
    """Columns instead of one object per point, nu-major (point i * len(u) + j is (nu[i], u[j])); dnu_trunc, a bound's
    ingredient and not a value, keeps 4 digits (rounded up): the file stays below the size of besselk_grid.json"""
    out = {"nu": GRID_NU, "u": GRID_U}
    assert [(r["nu"], r["u"]) for r in rows] == [(nu, u) for nu in GRID_NU for u in GRID_U]
    for k in ("M", "dM_du", "dM_dnu"):
        out[k] = [r[k] for r in rows]
    out["dnu_trunc"] = [float("%.3e" % (1.001 * r["dnu_trunc"])) for r in rows]          # rounded up
    with open(os.path.join(HERE, "matern_partials_grid.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))


# --------------------------------------------------------------------------- #
# the model, theta in mpmath (make_golden.loc_params / pair_value with nothing rounded to double on the way)
# --------------------------------------------------------------------------- #
def mp_theta(theta):
    """{aspect: [mpf] * p}; a -inf nugget intercept stays the float -inf"""
    return {k: [v if (isinstance(v, float) and math.isinf(v)) else mp.mpf(float(v)) for v in vs] for k, vs in theta.items()}


def perturbed(th, name, k, s):
    out = {a: list(v) for a, v in th.items()}
    if not (isinstance(out[name][k], float) and math.isinf(out[name][k])):
        out[name][k] = out[name][k] + s
    return out


def lin(xrow, b):
    return mp.fsum(x * c for x, c in zip(xrow, b))


def nugget_off(th):
    v = th["nugget"][0]
    return isinstance(v, float) and math.isinf(v)


def site_params(th, Xmp, smooth_limits):
    lo, hi = mp.mpf(float(smooth_limits[0])), mp.mpf(float(smooth_limits[1]))
    scale_je = [mp.mpf(0)] + list(th["scale"][1:])
    out = []
    for xr in Xmp:
        t = {}
        t["tilt"] = mp.pi / (1 + mp.exp(-lin(xr, th["tilt"])))
        t["rd"] = mp.exp(2 * lin(xr, scale_je))
        t["an"] = mp.exp(lin(xr, th["aniso"]))
        t["dets"] = t["rd"] * t["an"]
        t["sigma"] = mp.exp(lin(xr, th["std.dev"]) / 2)
        t["nugget"] = mp.mpf(0) if nugget_off(th) else mp.exp(lin(xr, th["nugget"]))
        t["nu"] = (hi - lo) / (1 + mp.exp(-lin(xr, th["smooth"]))) + lo
        t["diag"] = mp.exp(lin(xr, th["std.dev"])) + t["nugget"]
        t["rho"] = mp.exp(2 * lin(xr, th["scale"]))           # the taper model's range: the full scale vector
        out.append(t)
    return out


_KCACHE = {}


def matern_cached(nu, u):
    """Matern correlation; for u >= 706 the reference's stand-in (K_nu replaced by sqrt(pi / 2u) e^-u)"""
    key = (nu, u)
    m = _KCACHE.get(key)
    if m is None:
        k = mp.besselk(nu, u) if u < 706 else mp.sqrt(mp.pi / (2 * u)) * mp.exp(-u)
        m = mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(u, nu) * k
        _KCACHE[key] = m
    return m


def dense_pair(a, b, dx, dy, gr):
    """make_golden.pair_value (difference parameterisation), u returned beside the value"""
    s11 = (a["rd"] + b["rd"]) / 2
    s22 = (a["rd"] * a["an"] ** 2 + b["rd"] * b["an"] ** 2) / 2
    s12 = (a["rd"] * a["an"] * mp.cos(a["tilt"]) + b["rd"] * b["an"] * mp.cos(b["tilt"])) / 2
    det = s11 * s22 - s12 * s12
    nu = mp.sqrt(a["nu"]) * mp.sqrt(b["nu"])
    q = s22 * dx * dx + s11 * dy * dy - 2 * s12 * dx * dy
    u = mp.sqrt(8 * nu / (gr * det)) * mp.sqrt(q)
    if u == 0:
        return a["diag"], u, nu
    amp = mp.sqrt(a["dets"] * mp.sin(a["tilt"]) * b["dets"] * mp.sin(b["tilt"]))
    return matern_cached(nu, u) * a["sigma"] * b["sigma"] * amp / mp.sqrt(det), u, nu


def dense_sigma(th, locs_mp, Xmp, smooth_limits, stats=None):
    n = len(Xmp)
    lp = site_params(th, Xmp, smooth_limits)
    gr = mp.exp(2 * th["scale"][0])
    S = mp.zeros(n, n)
    for i in range(n):
        S[i, i] = lp[i]["diag"]
        for j in range(i + 1, n):
            v, u, nu = dense_pair(lp[i], lp[j], locs_mp[i][0] - locs_mp[j][0], locs_mp[i][1] - locs_mp[j][1], gr)
            S[i, j] = S[j, i] = v
            if stats is not None:
                stats.append((fl(u), fl(nu)))
    return S


def taper_sigma(th, locs_mp, Xmp, smooth_limits, pattern):
    """S = T o cov_rns_taper on the pattern (tests/grad_taper_reference.py's model; a coincident pair takes the diagonal
    value of its larger-index site)"""
    n = len(Xmp)
    lp = site_params(th, Xmp, smooth_limits)
    S = mp.zeros(n, n)
    for (i, j), t in pattern.items():
        if i == j:
            S[i, i] = t * lp[i]["diag"]
            continue
        if i < j:
            continue
        a, b = lp[i], lp[j]
        dx, dy = locs_mp[i][0] - locs_mp[j][0], locs_mp[i][1] - locs_mp[j][1]
        nu = mp.sqrt(a["nu"]) * mp.sqrt(b["nu"])
        u = mp.sqrt(8 * nu) * mp.sqrt(dx * dx + dy * dy) / mp.sqrt((a["rho"] + b["rho"]) / 2)
        if u == 0:
            v = a["diag"]                                   # i > j: the larger index
        else:
            v = 2 * mp.sqrt(a["rho"] * b["rho"]) / (a["rho"] + b["rho"]) * a["sigma"] * b["sigma"] * matern_cached(nu, u)
        S[i, j] = S[j, i] = t * v
    return S


def forward(L, B):
    """L^-1 B for the lower-triangular L, B a list of columns"""
    n = L.rows
    out = []
    for col in B:
        y = [mp.mpf(0)] * n
        for i in range(n):
            y[i] = (col[i] - mp.fsum(L[i, k] * y[k] for k in range(i))) / L[i, i]
        out.append(y)
    return out


def sq(y):
    return mp.fsum(v * v for v in y)


def dotv(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def gls(YX, YZ):
    """W = YX' YX, sum log diag chol(W), beta_k = W^-1 YX' YZ_k, the GLS quadratic forms"""
    q = len(YX)
    W = mp.matrix(q, q)
    for a in range(q):
        for b in range(q):
            W[a, b] = dotv(YX[a], YX[b])
    Lw = mp.cholesky(W)
    half = mp.fsum(mp.log(Lw[a, a]) for a in range(q))
    betas, quads = [], []
    for yz in YZ:
        g = mp.matrix([dotv(YX[a], yz) for a in range(q)])
        beta = mp.lu_solve(W, g)
        betas.append([beta[a] for a in range(q)])
        quads.append(sq(yz) - mp.fsum(g[a] * beta[a] for a in range(q)))
    return half, betas, quads


def objectives(S, Xmp, Zcols, mean, q, want_parts=False, mean_steps=False):
    """dense, Profile (Xb = the first q columns of X) and REML (Xb = X) -2 log-likelihoods of one Sigma"""
    n, p, r = len(Xmp), len(Xmp[0]), len(Zcols)
    L = mp.cholesky(S)
    half = mp.fsum(mp.log(L[i, i]) for i in range(n))
    Xcols = [[Xmp[i][k] for i in range(n)] for k in range(p)]
    Y = forward(L, Zcols + Xcols)
    YZ, YX = Y[:r], Y[r:]
    log2pi = mp.log(2 * mp.pi)

    def dense_value(m):
        # L^-1 (z - X m) = YZ - YX m
        quads = [sq([YZ[c][i] - mp.fsum(YX[k][i] * m[k] for k in range(p)) for i in range(n)]) for c in range(r)]
        return r * (n * log2pi + 2 * half) + mp.fsum(quads), quads

    fd, qd = dense_value(mean)
    hp, bp, qp = gls(YX[:q], YZ)
    hr, br, qr = gls(YX, YZ)
    out = {"dense": fd, "profile": r * (n * log2pi + 2 * half) + mp.fsum(qp),
           "reml": r * ((n - p) * log2pi + 2 * half + 2 * hr) + mp.fsum(qr)}
    if want_parts:
        def bmean(b, nb):
            return [mp.fsum(b[c][a] for c in range(r)) / r for a in range(nb)]
        out["parts"] = {"dense": [half] + qd, "profile": [half, hp] + qp + bmean(bp, q), "reml": [half, hr] + qr + bmean(br, p)}
    if mean_steps:
        d = step()
        out["grad_mean"] = []
        for k in range(p):
            mp_, mm = list(mean), list(mean)
            mp_[k] += d
            mm[k] -= d
            out["grad_mean"].append((dense_value(mp_)[0] - dense_value(mm)[0]) / (2 * d))
    return out


def taper_objective(S, Xmp, Zcols, mean, want_parts=False, mean_steps=False):
    n, p, r = len(Xmp), len(Xmp[0]), len(Zcols)
    L = mp.cholesky(S)
    half = mp.fsum(mp.log(L[i, i]) for i in range(n))
    Xcols = [[Xmp[i][k] for i in range(n)] for k in range(p)]
    Y = forward(L, Zcols + Xcols)
    YZ, YX = Y[:r], Y[r:]

    def quads(m):
        return [sq([YZ[c][i] - mp.fsum(YX[k][i] * m[k] for k in range(p)) for i in range(n)]) for c in range(r)]

    qd = quads(mean)
    out = {"logdet": r * 2 * half, "quad": mp.fsum(qd)}
    if want_parts:
        out["value"] = r * (n * mp.log(2 * mp.pi) + 2 * half) + mp.fsum(qd)
        out["parts"] = [half] + qd
    if mean_steps:
        d = step()
        out["grad_mean"] = []
        for k in range(p):
            mp_, mm = list(mean), list(mean)
            mp_[k] += d
            mm[k] -= d
            out["grad_mean"].append((mp.fsum(quads(mp_)) - mp.fsum(quads(mm))) / (2 * d))
    return out


# --------------------------------------------------------------------------- #
# cases
# --------------------------------------------------------------------------- #
def getscale(X):
    """cocons_amd.workloads.design_from_locs' standardisation of [1, x, y], restated (the generator imports no library code)"""
    out = X.copy()
    for k in range(1, X.shape[1]):
        out[:, k] = (X[:, k] - X[:, k].mean()) / X[:, k].std(ddof=1)
    return out


def design(locs):
    return getscale(np.column_stack([np.ones(locs.shape[0]), locs[:, 0], locs[:, 1]]))


def base_theta():
    return {"mean": [0.3, -0.15, 0.2], "std.dev": [0.0, 0.3, -0.2], "scale": [float(np.log(0.2)), 0.2, 0.1],
            "aniso": [0.0, 0.25, -0.25], "tilt": [0.0, 0.3, 0.3], "smooth": [0.0, 0.5, -0.5],
            "nugget": [float(np.log(1e-2)), 0.3, -0.2]}


def make_case(name):
    """locs, X, z, theta, smooth_limits, q (Profile's x_betas = X[:, :q]) of one dense-family case"""
    n, r, sl = 70, 1, [0.5, 2.5]
    th = base_theta()
    seed = {"base": 3, "tiles": 4, "wide": 5, "low": 6, "nonugget": 7, "far": 8, "nu1p5": 9, "nu1": 10}[name]
    rng = np.random.default_rng(seed)
    if name == "base":
        r = 2
    if name == "tiles":
        n = 140
    locs = rng.uniform(0, 1, size=(n, 2))
    if name == "far":               # 7 clusters of 10 sites: u of order 1 inside a cluster, beyond 706 between clusters
        centres = np.array([[0.1, 0.1], [0.9, 0.15], [0.5, 0.5], [0.15, 0.85], [0.85, 0.9], [0.5, 0.05], [0.05, 0.5]])
        locs = np.repeat(centres, 10, axis=0) + rng.uniform(0, 1, size=(n, 2)) * 4e-4
        th["scale"][0] = float(np.log(2e-4))
    if name == "base":
        locs[7] = locs[3]
    X = design(locs)
    if name == "base":
        X[7] = X[3] + [0.0, 0.5, 0.5]
    if name == "wide":
        sl = [0.1, 6.0]
        th["smooth"] = [0.0, 1.0, -1.0]
    if name == "low":
        sl = [0.05, 0.5]
    if name == "nonugget":
        th["nugget"] = [float("-inf"), 0.0, 0.0]
        th["scale"][0] = float(np.log(0.05))
    if name == "nu1p5":
        sl = [1.5, 1.5]
        th["smooth"] = [0.0, 0.0, 0.0]
    if name == "nu1":               # hi == lo on the general branch: a varying smooth vector with zero span
        sl = [1.0, 1.0]
    z = rng.standard_normal((n, r)) + 0.4 * X[:, [1]] - 0.2
    return dict(name=name, n=n, r=r, p=3, q=2, locs=locs, X=X, z=z, theta=th, smooth_limits=sl)


CASES = ("base", "tiles", "wide", "low", "nonugget", "far", "nu1p5", "nu1")


def make_taper_case():
    sys.path.insert(0, os.path.dirname(HERE))
    from grad_taper_reference import wendland1_pattern
    n, r = 150, 2
    rng = np.random.default_rng(1050)
    locs = rng.uniform(0, 1, size=(n, 2))
    locs[7] = locs[3]
    X = design(locs)
    X[7] = X[3]
    X[3] = X[3] + [0.0, 0.5, 0.0]            # the earlier of the two gets the larger variance: S stays positive definite
    th = base_theta()
    th["mean"] = [0.3, -0.2, 0.1]
    th["nugget"] = [float(np.log(1e-2)), 0.0, 0.0]
    z = rng.standard_normal((n, r))
    ci, rp, ent = wendland1_pattern(locs, TAPER_DELTA)
    rows = np.repeat(np.arange(n), np.diff(rp))
    pattern = {(int(i), int(j) - 1): mp.mpf(float(t)) for i, j, t in zip(rows, ci, ent)}
    return dict(name="taper", n=n, r=r, p=3, locs=locs, X=X, z=z, theta=th, smooth_limits=[0.5, 2.5], pattern=pattern,
                nnz=int(ci.size))


def as_mp(c):
    locs_mp = [[mp.mpf(float(v)) for v in row] for row in c["locs"]]
    Xmp = [[mp.mpf(float(v)) for v in row] for row in c["X"]]
    Zcols = [[mp.mpf(float(c["z"][i, k])) for i in range(c["n"])] for k in range(c["r"])]
    th = mp_theta(c["theta"])
    return locs_mp, Xmp, Zcols, th


def s60(x):
    return mp.nstr(x, DPS - 5)


def task(args):
    """One unit of work: ("base", case) or ("row", case, aspect, [k...]) -> strings of mpmath numbers"""
    mp.mp.dps = DPS
    _KCACHE.clear()
    kind, name = args[0], args[1]
    c = make_taper_case() if name == "taper" else make_case(name)
    locs_mp, Xmp, Zcols, th = as_mp(c)
    sl = c["smooth_limits"]
    taper = name == "taper"

    def evaluate(t, base=False, stats=None):
        if taper:
            S = taper_sigma(t, locs_mp, Xmp, sl, c["pattern"])
            return taper_objective(S, Xmp, Zcols, t["mean"], base, base), S
        S = dense_sigma(t, locs_mp, Xmp, sl, stats)
        return objectives(S, Xmp, Zcols, t["mean"], c["q"], base, base), S

    if kind == "base":
        stats = []
        o, S = evaluate(th, True, stats)
        Sf = np.array([[fl(S[i, j]) for j in range(c["n"])] for i in range(c["n"])])
        res = {"cond": float(np.linalg.cond(Sf)), "stats": stats}
        if not taper and name != "far":      # the same matrix from make_golden.mp_cov (theta in doubles, no stand-in)
            S0 = MG.mp_cov(c["theta"], c["locs"], c["X"], sl)
            assert max(abs(S[i, j] - S0[i, j]) for i in range(c["n"]) for j in range(c["n"])) < mp.mpf(10) ** (5 - DPS)
        for k, v in o.items():
            if k == "parts" and not taper:
                res[k] = {a: [s60(x) for x in b] for a, b in v.items()}
            elif isinstance(v, list):
                res[k] = [s60(x) for x in v]
            else:
                res[k] = s60(v)
        return args, res
    _, _, aspect, ks = args
    d = step()
    res = {}
    for k in ks:
        op, _ = evaluate(perturbed(th, aspect, k, d))
        om, _ = evaluate(perturbed(th, aspect, k, -d))
        keys = ("logdet", "quad") if taper else ("dense", "profile", "reml")
        res[k] = {a: s60((op[a] - om[a]) / (2 * d)) for a in keys}
    return args, res


def enc_theta(t):
    return {k: [("-inf" if (isinstance(v, float) and np.isneginf(v)) else v) for v in vs] for k, vs in t.items()}


def check_case(c, base):
    """the condition each case is there for"""
    name = c["name"]
    u = np.array([s[0] for s in base["stats"]])
    nu = np.array([s[1] for s in base["stats"]])
    if not name == "taper":
        assert base["cond"] <= 1e4, (name, base["cond"])
    if name == "base":
        assert np.sum(u == 0) == 1
    else:
        assert not np.any(u == 0)
    if name == "wide":
        assert nu.min() < 0.5 and nu.max() > 3.5, (nu.min(), nu.max())
    if name == "low":
        assert np.all(np.floor(nu + 0.5) == 0)
    if name == "far":
        frac = np.mean(u >= 706)
        assert 0.1 <= frac <= 0.9, frac


def generate(names):
    tasks = []
    for name in names:
        if name == "grid":
            continue
        rows = TAPER_ROWS if name == "taper" else ROWS
        tasks.append(("base", name))
        for a in rows:
            if name == "tiles" and a not in ("std.dev", "nugget"):
                tasks.extend(("row", name, a, [k]) for k in range(3))
            else:
                tasks.append(("row", name, a, [0, 1, 2]))
    weight = {"tiles": 4, "taper": 2}
    tasks.sort(key=lambda t: -weight.get(t[1], 1))
    results = {}
    with multiprocessing.Pool(WORKERS) as pool:
        if "grid" in names:
            rows = pool.map(grid_row, [(nu, u) for nu in GRID_NU for u in GRID_U], chunksize=8)
            write_grid(rows)
            print("matern_partials_grid.json: %d points" % len(rows), flush=True)
        for args, res in pool.imap_unordered(task, tasks):
            results.setdefault(args[1], {})
            if args[0] == "base":
                results[args[1]]["base"] = res
            else:
                results[args[1]].setdefault(args[2], {}).update(res)
            print("done", args, flush=True)
    for name in names:
        if name == "grid":
            continue
        res = results[name]
        base = res["base"]
        c = make_taper_case() if name == "taper" else make_case(name)
        rows = TAPER_ROWS if name == "taper" else ROWS

        def table(key):
            return [[float(mp.mpf(res[a][k][key])) if a in rows else 0.0 for k in range(3)] for a in ROWS]

        out = {"case": name, "n": c["n"], "r": c["r"], "p": c["p"], "locs": c["locs"].tolist(), "X": c["X"].tolist(),
               "z": c["z"].tolist(), "theta": enc_theta(c["theta"]), "smooth_limits": c["smooth_limits"]}
        if name == "taper":
            out["delta"] = TAPER_DELTA
            out["nnz"] = c["nnz"]
            out["cond"] = base["cond"]
            out["value"] = float(mp.mpf(base["value"]))
            out["parts"] = [float(mp.mpf(v)) for v in base["parts"]]
            out["grad_logdet"] = table("logdet")
            out["grad_quad"] = table("quad")
            out["grad_mean"] = [float(mp.mpf(v)) for v in base["grad_mean"]]
            fname = "grad_taper_n150.json"
        else:
            check_case(c, base)
            out["x_betas"] = c["X"][:, :c["q"]].tolist()
            out["cond"] = base["cond"]
            for obj in ("dense", "profile", "reml"):
                out[obj] = {"value": float(mp.mpf(base[obj])), "parts": [float(mp.mpf(v)) for v in base["parts"][obj]],
                            "grad_table": table(obj)}
            out["dense"]["grad_mean"] = [float(mp.mpf(v)) for v in base["grad_mean"]]
            out["reml"]["rank"] = c["p"]
            if name == "nonugget":
                assert all(v == 0.0 for o in ("dense", "profile", "reml") for v in out[o]["grad_table"][5])
            if name in ("nu1p5", "nu1"):
                assert all(v == 0.0 for o in ("dense", "profile", "reml") for v in out[o]["grad_table"][4])
            fname = "grad_dense_%s.json" % name
        out["ref_err"] = {}
        with open(os.path.join(HERE, fname), "w") as f:
            json.dump(out, f)
        print(fname, "cond %.3g" % out["cond"], flush=True)


# --------------------------------------------------------------------------- #
# ref_err: the float64 statements against the golden
# --------------------------------------------------------------------------- #
def dec_theta(t):
    return {k: np.array([(-np.inf if v == "-inf" else v) for v in vs], dtype=float) for k, vs in t.items()}


def family_errors(got_table, want_table, got_mean=None, want_mean=None):
    """{family: max |got - want| over the row / the row's largest |want|} (0 for a row that is zero in both)"""
    out = {}
    rows = list(zip(ROWS, np.asarray(got_table), np.asarray(want_table)))
    if want_mean is not None:
        rows.append(("mean", np.asarray(got_mean), np.asarray(want_mean)))
    for name, g, w in rows:
        scale = float(np.max(np.abs(w)))
        err = float(np.max(np.abs(g - w)))
        out[name] = (err / scale) if scale > 0 else (0.0 if err == 0 else float("inf"))
    return out


def reference_errors(fx):
    """the ref_err block of one loaded fixture"""
    import grad_profile_reference as GPR
    import grad_reference as GR
    import grad_taper_reference as GT
    th = dec_theta(fx["theta"])
    T = np.stack([th[k] for k in ROWS])
    locs, X, z, sl = np.array(fx["locs"]), np.array(fx["X"]), np.array(fx["z"]), tuple(fx["smooth_limits"])
    if fx["case"] == "taper":
        pat = GT.wendland1_pattern(locs, fx["delta"])
        f, parts, gl, gq, gm = GT.neg2loglik_taper_grad(T, th["mean"], locs, X, z, sl, pat)
        gol_l, gol_q = np.array(fx["grad_logdet"]), np.array(fx["grad_quad"])
        return {"total": family_errors(gl + gq, gol_l + gol_q, gm, fx["grad_mean"]),
                "logdet": family_errors(gl, gol_l), "quad": family_errors(gq, gol_q)}
    out = {}
    f, gt, gm = GR.neg2loglik_grad(T, th["mean"], locs, X, z, sl)
    out["dense"] = family_errors(gt, fx["dense"]["grad_table"], gm, fx["dense"]["grad_mean"])
    f, gt, beta, quad = GPR.profile_grad(th, locs, X, z, np.array(fx["x_betas"]), sl)
    out["profile"] = family_errors(gt, fx["profile"]["grad_table"])
    f, gt, beta, quad = GPR.reml_grad(th, locs, X, z, sl)
    out["reml"] = family_errors(gt, fx["reml"]["grad_table"])
    return out


def fixture_files():
    return ["grad_dense_%s.json" % c for c in CASES] + ["grad_taper_n150.json"]


def fill_ref_err():
    for fname in fixture_files():
        path = os.path.join(HERE, fname)
        if not os.path.exists(path):
            continue
        with open(path) as f:
            fx = json.load(f)
        fx["ref_err"] = reference_errors(fx)
        with open(path, "w") as f:
            json.dump(fx, f)
        for obj, fam in fx["ref_err"].items():
            print(fname, obj, " ".join("%s %.2e" % kv for kv in fam.items()), flush=True)


def main():
    argv = sys.argv[1:]
    if "--ref-err" in argv:
        fill_ref_err()
        return
    names = ["grid"] + list(CASES) + ["taper"]
    if "--only" in argv:
        names = argv[argv.index("--only") + 1:]
    generate(names)
    fill_ref_err()
    print("golden gradient vectors written")


if __name__ == "__main__":
    main()
