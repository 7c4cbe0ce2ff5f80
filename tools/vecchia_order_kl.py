"""What the order buys the approximation, on the CPU: python tools/vecchia_order_kl.py [--n 2500] [--out FILE].

Uniform sites on the unit square, the oracle's covariance for a stationary model (intercept only: std.dev 1, scale 0.15,
smoothness 1.5 -- the middle of the smooth limits --, nugget 1e-8), the exact m nearest earlier neighbours by the rule of the
device search (tests/knn_reference.brute_self).  For the sites as they come (a random order), for the exact greedy maxmin
order (every next point the one farthest from those chosen, from the point nearest the centre) and for host.vecchia_order
(the bits of cocons_vecchia_order): the KL divergence of the Vecchia model from the exact one,
    KL = sum_i log d_i - 1/2 log det Sigma
(d_i the conditional standard deviations; the trace term of the divergence is n for a Vecchia model built from Sigma itself).
No GPU is used.  Nothing is asserted; the lines also go to --out."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_reference as KR                  # noqa: E402
import vecchia_reference as VR              # noqa: E402
from cocons_amd import host                 # noqa: E402
from oracle import oracle as O              # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


N = int(_opt("--n", 2500))
OUT = _opt("--out", None)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def exact_maxmin(locs):
    c = 0.5 * (locs.min(axis=0) + locs.max(axis=0))
    first = int(np.argmin(np.sum((locs - c) ** 2, axis=1)))
    near = np.sum((locs - locs[first]) ** 2, axis=1)
    out = [first]
    near[first] = -1.0
    for _ in range(locs.shape[0] - 1):
        i = int(np.argmax(near))
        out.append(i)
        near = np.minimum(near, np.sum((locs - locs[i]) ** 2, axis=1))
        near[i] = -1.0
    return np.asarray(out)


O.build()
locs = np.random.default_rng(20260000 + N).uniform(0, 1, size=(N, 2))
X = np.ones((N, 1), order="F")
th = {"mean": np.zeros(1), "std.dev": np.zeros(1), "scale": np.array([np.log(0.15)]), "aniso": np.zeros(1), "tilt": np.zeros(1),
      "smooth": np.zeros(1), "nugget": np.array([np.log(1e-8)])}
orders = {"random order": np.arange(N), "exact greedy maxmin": exact_maxmin(locs),
          "host.vecchia_order": host.vecchia_order(locs).astype(np.int64) - 1}
say("python tools/vecchia_order_kl.py --n %d" % N)
for m in (30, 20, 10):
    row = []
    for name, o in orders.items():
        l = np.ascontiguousarray(locs[o])
        S = O.cov_rns(th, l, X, (0.5, 2.5))
        half_logdet = float(np.sum(np.log(np.diag(np.linalg.cholesky(S)))))
        logd = VR.whiten(S, KR.brute_self(l, m), np.zeros((N, 1)))[1]
        row.append("%s %.3f" % (name, float(np.sum(logd)) - half_logdet))
    say("n = %d, m = %d, KL of the Vecchia model from the exact one: %s" % (N, m, "; ".join(row)))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
