"""The persistent launch's tile product streams its operands through a ring of LDS-DMA stages (chol.hip dag_kernel): the
same MFMAs in the same ascending-k order as the register-staged chunks it replaced, so every value is bit-identical to the
one that build gave.  tests/golden/dag_pipeline_bits.json holds those values (written by the register-staged build with
`python tests/test_gpu_dag_pipeline.py --write`); the sizes exercise every K a task uses (64 and 128 for the panel tasks,
128 for the split halves, 256 for the update tiles), a last block of one tile, no padding, and the head-only form (a three-step
head at n = 4096, the default threshold at n = 10^4)."""
import json
import math
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dag_pipeline_bits.json")

# (gx, gy, dag_min_tiles): n = 700 (6 tiles), 2115 (17 tiles: a last block of one tile), 4096 (32 tiles, no padding) with the
# DAG schedule for every step, the head only at n = 4096 (a three-step head) and at n = 10^4 (the default threshold)
CASES = [(28, 25, 0), (45, 47, 0), (64, 64, 0), (64, 64, 1000), (100, 100, 2000)]


def _tune(name, value):
    from cocons_amd import _lib
    L = _lib.load()
    _lib.check(L.cocons_debug_tune(name.encode(), int(value)), "cocons_debug_tune")


def _problem(gx, gy):
    from cocons_amd import workloads as wl
    xs, ys = np.linspace(0, 1, gx), np.linspace(0, 1, gy)
    locs = np.array([(x, y) for y in ys for x in xs])
    X = wl.design_from_locs(locs)["std.covs"]
    th = wl.theta_full()
    th["mean"] = np.array([0.1, -0.2, 0.05])
    n = locs.shape[0]
    rng = np.random.default_rng(n)
    z = rng.standard_normal((n, 2)) + (X @ np.array([0.2, 0.3, -0.1]))[:, None]
    return locs, X, th, z


def evaluate(gx, gy, min_tiles, reps=3):
    """-2 log-likelihood and its parts under the DAG schedule, `reps` times on one handle: the list of (value, parts), the
    engine state and the stage profile of the last evaluation."""
    import cocons_amd as ca
    from cocons_amd import workloads as wl
    locs, X, th, z = _problem(gx, gy)
    fit = ca.CoconsFit(locs, X, z, wl.SMOOTH_LIMITS)
    _tune("dag", 1)
    _tune("dag_min_tiles", min_tiles)
    try:
        out = [fit.neg2loglik_core(th) for _ in range(reps)]
        st = fit.profile_stages(th, reps=1)
        es = fit.engine_state()
    finally:
        _tune("dag", int(os.environ.get("COCONS_DAG", "1")))
        _tune("dag_min_tiles", int(os.environ.get("COCONS_DAG_MIN_TILES", "2000")))
        fit.close()
    return out, es, st


def _key(gx, gy, min_tiles):
    return "%dx%d/min%d" % (gx, gy, min_tiles)


def _bits(v, parts):
    return {"value": float(v).hex(), "parts": [float(p).hex() for p in np.asarray(parts, dtype=np.float64).ravel()]}


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("COCONS_ENGINE", "1") == "0",
                    reason="COCONS_ENGINE=0: the dependency-driven schedule needs the diagonal-block engine")
@pytest.mark.parametrize("gx,gy,min_tiles", CASES)
def test_dag_pipeline_same_bits(oracle, gx, gy, min_tiles):
    """Every evaluation equals the register-staged build's value and parts bit for bit, repeated evaluations too; the DAG
    launch really ran; no hand-off timed out; against the CPU oracle to 1e-9 where it finishes in seconds."""
    from cocons_amd import workloads as wl
    with open(GOLDEN) as f:
        want = json.load(f)[_key(gx, gy, min_tiles)]
    out, es, st = evaluate(gx, gy, min_tiles)
    for v, parts in out:
        assert _bits(v, parts) == want, (v, float.fromhex(want["value"]))
    assert es["retries"] == 0 and es["active"], es
    assert st["dag_ms"] > 0 and st["dag_flops"] > 0
    locs, X, th, z = _problem(gx, gy)
    n = locs.shape[0]
    if n <= 2400:
        S = oracle.cov_rns(th, locs, X, wl.SMOOTH_LIMITS)
        info, ld, quad, _ = oracle.chol_ld(S, z - (X @ th["mean"])[:, None])
        ref = sum(n * math.log(2 * math.pi) + 2 * ld + float(quad[k]) for k in range(2))
        assert abs(out[0][0] - ref) <= 1e-9 * abs(ref)


if __name__ == "__main__":
    # python tests/test_gpu_dag_pipeline.py --write [PATH]: record the values of CASES with the build that is loaded
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:2] != ["--write"]:
        sys.exit("usage: test_gpu_dag_pipeline.py --write [PATH]")
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    rec = {}
    for gx, gy, mt in CASES:
        out, es, st = evaluate(gx, gy, mt)
        assert all(_bits(*o) == _bits(*out[0]) for o in out) and es["retries"] == 0 and st["dag_ms"] > 0, (gx, gy, mt)
        rec[_key(gx, gy, mt)] = _bits(*out[0])
        print(_key(gx, gy, mt), rec[_key(gx, gy, mt)]["value"], flush=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
