"""What neighbours by model correlation buy the approximation, on the CPU: python tools/vecchia_corr_kl.py [--n 2500] [--m 30]
[--out FILE].

Uniform sites on the unit square, the oracle's covariance, the sites as they come (a random order) and in the maxmin order
of host.vecchia_order (the bits of cocons_vecchia_order).  For the Euclidean table of width m (tests/knn_reference.brute_self,
the rule of the device search) and for the tables of host.vecchia_neighbours_corr (the rule of cocons_vecchia_neighbours_corr,
DESIGN.md 4af) at (m_cand, hops) = (60, 1), (30, 2), (60, 2) -- stated at m = 30 and scaled in proportion at another m --: the
KL divergence of the Vecchia model from the exact one,
    KL = sum_i log d_i - 1/2 log det Sigma
(d_i the conditional standard deviations), its ratio to the Euclidean table's, and the mean number of unique candidates a row
ranks.  Three thetas (tests/corr_knn_reference.py): the stationary isotropic setting of tools/vecchia_order_kl.py, where every
table must be the Euclidean one as sets; a global geometric anisotropy of axis ratio 5; anisotropy, tilt and range driven by
the covariates.  No GPU is used.  Nothing is asserted; the lines also go to --out."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import corr_knn_reference as CR             # noqa: E402
import knn_reference as KR                  # noqa: E402
from cocons_amd import host, workloads as wl     # noqa: E402
from oracle import oracle as O              # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


N = int(_opt("--n", 2500))
M = int(_opt("--m", 30))
OUT = _opt("--out", None)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def unique_candidates(cand, hops):
    """mean over the rows of the number of indices the re-ranking evaluates"""
    total = 0
    for i in range(cand.shape[0]):
        c = cand[i][cand[i] > 0]
        if hops == 2 and c.size:
            c = np.concatenate([c, cand[c - 1].ravel()])
        total += np.unique(c[c > 0]).size
    return total / cand.shape[0]


O.build()
locs0 = np.random.default_rng(20260000 + N).uniform(0, 1, size=(N, 2))
X3 = np.asfortranarray(wl.design_from_locs(locs0)["std.covs"])
X1 = np.ones((N, 1), order="F")
thetas = (("isotropic (tools/vecchia_order_kl.py's)", CR.theta_iso(), X1),
          ("global anisotropy, axis ratio 5, nugget 0.01", CR.theta_aniso(), X1),
          ("covariate-driven anisotropy, tilt and range, nugget 0.01", CR.theta_covariate(), X3))
orders = (("random order", np.arange(N)), ("maxmin order", host.vecchia_order(locs0).astype(np.int64) - 1))
say("python tools/vecchia_corr_kl.py --n %d --m %d" % (N, M))
for oname, o in orders:
    locs = np.ascontiguousarray(locs0[o])
    tables = {"euclid": KR.brute_self(locs, M)}
    for m_cand, hops in CR.SETTINGS:
        tables[CR.scaled(m_cand, M)] = KR.brute_self(locs, CR.scaled(m_cand, M))
    for tname, th, X in thetas:
        S = O.cov_rns(th, locs, np.asfortranarray(X[o]), wl.SMOOTH_LIMITS)
        half_logdet = float(np.sum(np.log(np.diag(np.linalg.cholesky(S)))))
        base = CR.kl(S, tables["euclid"], half_logdet)
        say("n = %d, m = %d, %s, %s: KL of the Euclidean table %.3f" % (N, M, oname, tname, base))
        want = [frozenset(r[r > 0]) for r in tables["euclid"]]
        for m_cand, hops in CR.SETTINGS:
            mc = CR.scaled(m_cand, M)
            nn = host.vecchia_neighbours_corr(S, tables[mc], M, hops)
            differ = sum(frozenset(r[r > 0]) != w for r, w in zip(nn, want))
            k = CR.kl(S, nn, half_logdet)
            say("    m_cand = %2d, hops = %d: KL %8.3f = %.3f of the Euclidean table's; %6.1f unique candidates a row; %d rows "
                "differ from the Euclidean table as sets" % (mc, hops, k, k / base, unique_candidates(tables[mc], hops), differ))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
