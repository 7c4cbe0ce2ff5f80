"""The float64 statements of the gradients (tests/grad_reference.py, grad_profile_reference.py, grad_taper_reference.py) against
the exact-arithmetic golden vectors of tests/golden/make_golden_grad.py -- without a GPU.

The golden gradients are 70-digit central differences of the whole objective: they share no algebra with the statements.
Per family (a row of the 6 x p table; the mean vector is a family of its own)

    e_ref = max |reference - golden| over the row / the row's largest |golden| component

must stay below 1e-11 for the five families without an order derivative and for the mean: cond(Sigma) eps is 1e4 x 1e-16 at
most (every fixture stores cond(Sigma) <= 1e4) and an order of magnitude is left to spare.  The smooth family must stay
below 1e-8: scipy's kv, good to about 1e-13, is divided by the step 1e-3 nu of the statement's difference in nu.  The
measured values are written into each fixture's ref_err block by `make_golden_grad.py --ref-err` (never by a test run); the
GPU tests take their bounds from that block (tests/test_gpu_grad_golden.py).  Measured: at most 5.2e-13 (tilt, limits (0.1, 6)) and 1.7e-10 (smooth)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import grad_reference as GR  # noqa: E402
import make_golden_grad as MGG  # noqa: E402

FAMILIES = MGG.ROWS + ("mean",)
BOUND = {f: 1e-11 for f in FAMILIES}
BOUND["smooth"] = 1e-8
LARGEST_FIXTURE = "besselk_grid.json"


def load(fname):
    with open(os.path.join(HERE, "golden", fname)) as f:
        return json.load(f)


def _check_block(fname, block):
    for obj, fams in block.items():
        for fam, e in fams.items():
            print("%s %s %-8s e_ref %.3e" % (fname, obj, fam, e))
            assert e <= BOUND[fam], (fname, obj, fam, e)


@pytest.mark.parametrize("fname", MGG.fixture_files())
def test_float64_statements_against_golden(fname):
    fx = load(fname)
    measured = MGG.reference_errors(fx)
    _check_block(fname, measured)
    # the committed block: filled, over the same objectives and families, within the same bounds
    stored = fx["ref_err"]
    assert {k: sorted(v) for k, v in stored.items()} == {k: sorted(v) for k, v in measured.items()}
    _check_block(fname + " (stored)", stored)


@pytest.mark.parametrize("fname", MGG.fixture_files())
def test_float64_values_against_golden(fname):
    """value and parts of the statements: 1e-12 relative (sums of n logarithms and quadratic forms at cond <= 1e4)"""
    import grad_profile_reference as GPR
    import grad_taper_reference as GT
    fx = load(fname)
    th = MGG.dec_theta(fx["theta"])
    T = np.stack([th[k] for k in MGG.ROWS])
    locs, X, z, sl = np.array(fx["locs"]), np.array(fx["X"]), np.array(fx["z"]), tuple(fx["smooth_limits"])
    if fx["case"] == "taper":
        f, parts, _, _, _ = GT.neg2loglik_taper_grad(T, th["mean"], locs, X, z, sl, GT.wendland1_pattern(locs, fx["delta"]))
        assert GT.wendland1_pattern(locs, fx["delta"])[0].size == fx["nnz"]
        assert abs(f - fx["value"]) <= 1e-12 * abs(fx["value"])
        assert np.max(np.abs(parts - fx["parts"]) / np.abs(fx["parts"])) <= 1e-12
        return
    f = GR.neg2loglik_grad(T, th["mean"], locs, X, z, sl)[0]
    assert abs(f - fx["dense"]["value"]) <= 1e-12 * abs(fx["dense"]["value"])
    r = fx["r"]
    for obj, res in (("profile", GPR.profile_grad(th, locs, X, z, np.array(fx["x_betas"]), sl)),
                     ("reml", GPR.reml_grad(th, locs, X, z, sl))):
        f, _, beta, quad = res
        gold = fx[obj]
        assert abs(f - gold["value"]) <= 1e-12 * abs(gold["value"]), obj
        assert np.max(np.abs(quad - gold["parts"][2:2 + r]) / np.abs(gold["parts"][2:2 + r])) <= 1e-12, obj
        want = np.array(gold["parts"][2 + r:])
        assert np.max(np.abs(beta.mean(axis=1) - want)) <= 1e-12 * np.max(np.abs(want)), obj


def test_fixture_conditions():
    """what each case is there for, read back from the committed numbers"""
    limit = os.path.getsize(os.path.join(HERE, "golden", LARGEST_FIXTURE))
    for fname in MGG.fixture_files() + ["matern_partials_grid.json"]:
        assert os.path.getsize(os.path.join(HERE, "golden", fname)) <= limit, fname
    for case in MGG.CASES:
        fx = load("grad_dense_%s.json" % case)
        assert fx["cond"] <= 1e4, (case, fx["cond"])
        locs = np.array(fx["locs"])
        coincident = sum(1 for i in range(fx["n"]) for j in range(i) if np.array_equal(locs[i], locs[j]))
        assert coincident == (1 if case == "base" else 0)
        for obj in ("dense", "profile", "reml"):
            g = np.array(fx[obj]["grad_table"])
            assert g.shape == (6, 3) and np.all(np.isfinite(g))
            assert np.all(g[5] == 0) == (case == "nonugget"), (case, obj)
            assert np.all(g[4] == 0) == (case in ("nu1p5", "nu1")), (case, obj)
    assert load("grad_dense_tiles.json")["n"] == 140
    assert load("grad_dense_nonugget.json")["theta"]["nugget"][0] == "-inf"
    lo, hi = load("grad_dense_low.json")["smooth_limits"]
    assert hi <= 0.5                                                 # nu_ij = sqrt(nu_i nu_j) < 1/2: matern_pair's n == 0
    tp = load("grad_taper_n150.json")
    assert np.all(np.array(tp["grad_logdet"])[2:4] == 0) and np.all(np.array(tp["grad_quad"])[2:4] == 0)


def test_scipy_matern_partials_on_the_grid_report():
    """grad_reference.matern_and_partials (scipy kv / kvp, Richardson in nu) on the golden grid: a report, so that the scipy
    statement's own accuracy is on record.  Nothing is asserted beyond the grid's shape."""
    g = load("matern_partials_grid.json")
    nu = np.repeat(np.array(g["nu"]), len(g["u"]))
    u = np.tile(np.array(g["u"]), len(g["nu"]))
    assert 600 <= nu.size <= 900 and all(len(g[k]) == nu.size for k in ("M", "dM_du", "dM_dnu", "dnu_trunc"))
    with np.errstate(all="ignore"):
        M, Mu, Mn = GR.matern_and_partials(nu, u)
    for name, got, key in (("M", M, "M"), ("dM/du", Mu, "dM_du"), ("dM/dnu", Mn, "dM_dnu")):
        want = np.array(g[key])
        ok = np.abs(want) > 1e-290
        rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
        rel = np.where(np.isfinite(rel), rel, np.inf)
        k = int(np.argmax(rel))
        print("scipy %-6s: median relative error %.2e, largest %.2e at nu = %g, u = %g; above 1e-8 at %d of %d points"
              % (name, np.median(rel), rel[k], nu[ok][k], u[ok][k], int(np.sum(rel > 1e-8)), rel.size))
