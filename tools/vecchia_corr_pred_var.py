"""What neighbours by model correlation buy local kriging, on the CPU: python tools/vecchia_corr_pred_var.py [--n 2500] [--mp 400]
[--m 30] [--out FILE].

Uniform observations and new sites on the unit square, the oracle's covariance.  For the Euclidean table of width m
(tests/knn_reference.brute_pred, the rule of the device search) and for the tables of host.vecchia_neighbours_corr_pred (the
rule of cocons_vecchia_neighbours_corr_pred) at (m_cand, hops) = (60, 1), (30, 2), (60, 2) -- stated at m = 30
and scaled in proportion at another m --: the mean and the worst, over the new sites, of
    (local-kriging variance on the table) / (exact kriging variance on all observations) - 1,
the mean number of unique candidates a site ranks, and the sites whose set differs from the Euclidean one.  Three thetas
(tests/corr_knn_reference.py): the stationary isotropic setting, where every table must be the Euclidean one as sets; a global
geometric anisotropy of axis ratio 5; anisotropy, tilt and range driven by the covariates.  No GPU is used.  Nothing is
asserted; the lines also go to --out."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import corr_knn_pred_reference as PR        # noqa: E402
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
MP = int(_opt("--mp", 400))
M = int(_opt("--m", 30))
OUT = _opt("--out", None)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def unique_candidates(first, lists, hops):
    total = 0
    for q in range(first.shape[0]):
        c = first[q][first[q] > 0]
        if hops == 2 and c.size:
            c = np.concatenate([c, lists[c - 1].ravel()])
        total += np.unique(c[c > 0]).size
    return total / first.shape[0]


O.build()
rng = np.random.default_rng(20260000 + N)
locs, q = rng.uniform(0, 1, size=(N, 2)), rng.uniform(0, 1, size=(MP, 2))
sc = wl.design_from_locs(locs)
X3 = np.asfortranarray(sc["std.covs"])
Xp3 = np.asfortranarray(wl.design_from_locs(q, sc["mean.vector"], sc["sd.vector"])["std.covs"])
X1, Xp1 = np.ones((N, 1), order="F"), np.ones((MP, 1), order="F")
thetas = (("isotropic (tools/vecchia_order_kl.py's)", CR.theta_iso(), X1, Xp1),
          ("global anisotropy, axis ratio 5, nugget 0.01", CR.theta_aniso(), X1, Xp1),
          ("covariate-driven anisotropy, tilt and range, nugget 0.01", CR.theta_covariate(), X3, Xp3))
say("python tools/vecchia_corr_pred_var.py --n %d --mp %d --m %d" % (N, MP, M))
euclid = KR.brute_pred(locs, q, M)
tables = {}
for m_cand, hops in PR.SETTINGS:
    mc = CR.scaled(m_cand, M)
    tables[mc] = (KR.brute_pred(locs, q, mc), KR.brute_pred(locs, locs, mc))
want = [frozenset(r[r > 0]) for r in euclid]
for tname, th, X, Xp in thetas:
    sl = wl.SMOOTH_LIMITS
    S = O.cov_rns(th, locs, X, sl)
    Cp = O.cov_rns_pred(th, locs, q, X, Xp, sl)
    dq = np.diagonal(O.cov_rns_pred(th, q, q, Xp, Xp, sl)).copy()
    d = np.diagonal(O.cov_rns_pred(th, locs, locs, X, X, sl)).copy()
    var = 1 / np.exp(-(Xp @ th["std.dev"])) + np.exp(Xp @ th["nugget"])
    base = PR.excess_variance(S, Cp, var, euclid)
    say("n = %d, %d new sites, m = %d, %s: excess variance of the Euclidean table mean %.3e worst %.3e" % ((N, MP, M, tname) + base))
    for m_cand, hops in PR.SETTINGS:
        mc = CR.scaled(m_cand, M)
        nn = host.vecchia_neighbours_corr_pred(Cp, dq, d, tables[mc][0], tables[mc][1], M, hops)
        differ = sum(frozenset(r[r > 0]) != w for r, w in zip(nn, want))
        ex = PR.excess_variance(S, Cp, var, nn)
        say("    m_cand = %2d, hops = %d: mean %.3e worst %.3e; %6.1f unique candidates a site; %d sites differ from the "
            "Euclidean table as sets" % (mc, hops, ex[0], ex[1], unique_candidates(tables[mc][0], tables[mc][1], hops), differ))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
