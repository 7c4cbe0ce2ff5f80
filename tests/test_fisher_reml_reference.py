"""The numpy / scipy statement of the REML fit's expected information (tests/fisher_reml_reference.py) without a GPU: the
projector form against the definition by error contrasts, the exact identity I_R(v_s, v_s) = r (n - rank X) / 2 (P Sigma P = P
and tr(P Sigma) = n - rank X), P X = 0, positive definiteness over the 18 unit directions, and the distance to the ML
information -- what a device path that forgot the projector would return.  Bounds: a decade over what float64 gives here
(DESIGN.md 4k lists the figures)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference as FR  # noqa: E402
import fisher_reml_reference as RR  # noqa: E402
from test_fisher_reference import _setup  # noqa: E402

from cocons_amd import host, workloads as wl  # noqa: E402

SIZES = (300, 130)


@functools.lru_cache(maxsize=None)
def _reference(n):
    """(X, Sigma, Sigma_a for the 18 unit directions and v_s) of the n-site problem with the coincident pair"""
    locs, X, th = _setup(n)
    dirs = np.concatenate([np.eye(18).reshape(18, 6, 3), FR.scaling_direction(3)[None]])
    S, Sa = FR.sigma_and_directions(host.theta_table(th), locs, X, wl.SMOOTH_LIMITS, dirs)
    for a in (X, S, Sa):
        a.setflags(write=False)
    return X, S, Sa


@pytest.mark.parametrize("n", SIZES)
def test_projector_annihilates_the_design(n):
    X, S, _ = _reference(n)
    P = RR.projector(S, X)
    gap = np.max(np.abs(P @ X)) / (np.max(np.abs(P)) * np.max(np.abs(X)))
    print("n=%d max |P X| = %.2e (%.2e of max |P| max |X|)" % (n, np.max(np.abs(P @ X)), gap))
    assert gap <= 2e-14                            # (seen: 1.4e-15 at n = 300, 4.7e-16 at n = 130)
    K = RR.contrast_basis(X)
    assert K.shape == (n, n - 3)
    assert np.max(np.abs(K.T @ X)) <= 1e-12 * np.max(np.abs(X))


@pytest.mark.parametrize("r", (1, 3))
@pytest.mark.parametrize("n", SIZES)
def test_two_forms_identity_definiteness_and_distance_to_ml(n, r):
    X, S, Sa = _reference(n)
    I1, I2 = RR.info_projector(S, Sa, X, r), RR.info_contrasts(S, Sa, X, r)
    gap = FR.metric(I1, I2)
    d = np.sqrt(np.diag(I1)[:18])
    lam = np.linalg.eigvalsh(I1[:18, :18] / np.outer(d, d))[0]
    ml = FR.info_solve(S, Sa, r)
    far = min(FR.metric(I1[:18, :18], ml[:18, :18]), FR.metric(ml[:18, :18], I1[:18, :18]))
    print("n=%d r=%d the two forms: %.2e; I_R(v_s, v_s) - r (n - 3) / 2 = %.2e, %.2e; smallest eigenvalue of the normalised "
          "matrix %.3g; distance to the ML information %.3g"
          % (n, r, gap, I1[18, 18] - r * (n - 3) / 2, I2[18, 18] - r * (n - 3) / 2, lam, far))
    assert gap <= 1e-12                            # (seen: 8.0e-14 at both sizes)
    for I in (I1, I2):
        assert abs(I[18, 18] - r * (n - 3) / 2) <= 2e-14 * r * n      # (seen: 1.3e-15 r n at n = 300)
        assert np.max(np.abs(I - I.T)) <= 1e-12 * np.max(np.abs(I))
    assert lam > 0                                 # (seen: 0.041 at n = 300, 0.054 at n = 130)
    # three decades over the GPU tests' 1e-7: an implementation without the projector cannot pass them
    assert far >= 1e-4                             # (seen: 0.34 at n = 300, 0.42 at n = 130)
