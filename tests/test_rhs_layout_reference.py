"""tests/rhs_layout_reference.py (the reference of tests/test_gpu_rhs_layouts.py) against the oracle's literal restatements of
the R closures -- GetNeg2loglikelihood, ...Profile and ...REML with lambda = (0, 0, 0) -- at n = 150 with many
realisations and with a wide x_betas, and its own refusals.  No GPU."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rhs_layout_reference as RL  # noqa: E402

SL = (0.5, 2.5)
LAM = (0.0, 0.0, 0.0)


def _par_pos_all_free(p):
    pp = OrderedDict()
    for k in ("mean", "std.dev", "scale", "aniso", "tilt", "smooth", "nugget"):
        pp[k] = [True] * p
    return pp


def _theta_vector(th, pp):
    """inverse of getModelLists(type = "diff") with every entry free"""
    raw = {k: np.array(v, float) for k, v in th.items()}
    sd, sc = raw["std.dev"].copy(), raw["scale"].copy()
    raw["std.dev"], raw["scale"] = sd + sc, sd - sc
    return np.concatenate([raw[k] for k in pp])


@pytest.mark.parametrize("r,q", [(5, 4), (20, 1)])
def test_reference_equals_the_literal_closures(oracle, r, q):
    n, p = 150, q
    locs, X, th, z = RL.layout_problem(n, p, r, 4100 + r)
    pp = _par_pos_all_free(p)
    tv = _theta_vector(th, pp)
    tl = oracle.getModelLists(tv, pp, "diff")
    for k in th:
        assert np.allclose(tl[k], th[k], rtol=0, atol=1e-15)
    v, parts = RL.dense(oracle, tl, locs, X, z, SL)
    want = oracle.GetNeg2loglikelihood(tv, pp, locs, X, SL, z, n, LAM, safe=False)
    print("dense r=%d q=%d: %.2e" % (r, q, abs(v - want) / abs(want)))
    assert abs(v - want) <= 1e-9 * abs(want)
    assert parts.shape == (1 + r,)
    assert abs(n * r * np.log(2 * np.pi) + 2 * r * parts[0] + parts[1:].sum() - v) <= 1e-12 * abs(v)
    v, parts, cond = RL.profile(oracle, tl, locs, X, z, X, SL)
    want = oracle.GetNeg2loglikelihoodProfile(tv, pp, locs, X, SL, z, n, X, LAM, safe=False)
    print("profile r=%d q=%d: %.2e %s" % (r, q, abs(v - want) / abs(want), cond))
    assert abs(v - want) <= 1e-9 * abs(want)
    assert parts.shape == (2 + r + q,)
    # the GLS coefficients: the literal formula of R/optim.R:329-341
    S = oracle.cov_rns(tl, locs, X, SL)
    V = np.linalg.solve(S, X)
    beta = np.linalg.solve(X.T @ V, V.T) @ z.sum(axis=1) / r
    assert np.max(np.abs(parts[2 + r:] - beta)) <= 1e-9 * np.max(np.abs(beta))
    vr, parts_r, cond = RL.profile(oracle, tl, locs, X, z, None, SL, reml=True)
    want = oracle.GetNeg2loglikelihoodREML(tv, pp, locs, X, X, SL, z, n, LAM, safe=False)
    print("reml r=%d q=%d: %.2e" % (r, q, abs(vr - want) / abs(want)))
    assert abs(vr - want) <= 1e-9 * abs(want)
    assert np.array_equal(parts_r[2:], parts[2:]) and parts_r[0] == parts[0]      # x_betas = X: the same Gram matrix
    rank = np.linalg.matrix_rank(X)
    assert abs((vr - v) - r * (2 * parts_r[1] - rank * np.log(2 * np.pi))) <= 1e-10 * abs(v)


def test_reference_refuses_what_it_cannot_vouch_for(oracle):
    """A quadratic form that cancels (one observation, an intercept: z' P z = 0) and a singular matrix are refused."""
    locs, X, th, z = RL.layout_problem(1, 1, 3, 4200)
    with pytest.raises(AssertionError):
        RL.profile(oracle, th, locs, X, z, X, SL)
    _, parts, cond = RL.profile(oracle, th, locs, X, z, X, SL, check=False)
    assert cond["ratio"] > 0.5 and parts.shape == (2 + 3 + 1,)
    locs, X, th, z = RL.layout_problem(40, 2, 3, 4201)
    bad = OrderedDict((k, np.array(v, float)) for k, v in th.items())
    bad["std.dev"][0] = -np.inf
    bad["nugget"][0] = -np.inf
    with pytest.raises(AssertionError):
        RL.dense(oracle, bad, locs, X, z, SL)
