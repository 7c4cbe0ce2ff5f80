"""The deeper ring of the tapered joint prediction (tests/krige_taper_joint_reference.py) against dense algebra, on the CPU:
for every depth the accumulated S_uu - sum_g V_g V_g' is S_uu - C (L L')^-1 C', the ring never holds more than
min(W + D - 1, nt) tile columns, no slot is taken over before its group's product has read it, and the loads are those
of the plain ring."""
import numpy as np
import pytest

from krige_taper_joint_reference import SlotOverwritten, ring_schur
from krige_taper_reference import load_schedule
from test_krige_taper_reference import T, _case, _rows


def _problem(name):
    rng, n, nt, A, L, hi, W = _case(name)
    ci, val = _rows(rng, n, nt)
    C = np.zeros((len(ci), n))
    for i, (c, v) in enumerate(zip(ci, val)):
        C[i, c] = v
    G = rng.standard_normal((len(ci), len(ci)))
    S_uu = G @ G.T + 5.0 * np.eye(len(ci))
    return nt, A, L, hi, W, ci, val, C, S_uu


@pytest.mark.parametrize("name", ["irregular", "narrow", "full", "single"])
def test_every_depth_gives_the_predictive_covariance(name):
    nt, A, L, hi, W, ci, val, C, S_uu = _problem(name)
    want = S_uu - C @ np.linalg.solve(A, C.T)
    for D in (1, 2, 3, W, W + 2):
        S, loads, width, groups = ring_schur(L, hi, T, W, D, ci, val, S_uu)
        assert np.max(np.abs(S - want)) <= 1e-12 * np.max(np.abs(want)), (name, D)
        assert width == min(W + D - 1, nt) * T, (name, D)            # never rows x n while W + D - 1 < nt
        assert loads == load_schedule(nt, W), (name, D)              # the live window stays W
        # the groups tile [0, nt) in order, D tile columns each but the last
        assert groups[0][0] == 0 and groups[-1][1] == nt
        assert all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
        assert all(g1 - g0 == D for g0, g1 in groups[:-1]) and 0 < groups[-1][1] - groups[-1][0] <= D
    if name in ("irregular", "narrow"):
        assert W + 3 - 1 < nt                                        # the deeper ring still wraps at D = 3


def test_row_without_entries_keeps_its_row_of_s_uu():
    nt, A, L, hi, W, ci, val, C, S_uu = _problem("irregular")
    S = ring_schur(L, hi, T, W, 2, ci, val, S_uu)[0]
    assert np.array_equal(S[3], S_uu[3]) and np.array_equal(S[:, 3], S_uu[:, 3])


def test_the_slot_a_load_takes_over_has_been_consumed():
    """Slot (J + W - 1) mod (W + D - 1) held tile J - D, whose group ended at step D floor((J - D) / D) + D - 1 <= J - 1."""
    for nt, W in ((13, 3), (16, 2), (9, 4), (40, 5)):
        for D in range(1, 9):
            Wr = min(W + D - 1, nt)
            for J, I in load_schedule(nt, W):
                prev = I - Wr
                if prev >= 0:
                    assert Wr == W + D - 1 and prev == J - D
                    assert D * (prev // D) + D - 1 <= J - 1, (nt, W, D, J)


def test_the_instrumented_ring_catches_a_ring_that_is_too_shallow():
    """The same loop with one slot fewer than the depth needs: a load meets a solved tile column whose product is pending."""
    nt, A, L, hi, W, ci, val, C, S_uu = _problem("narrow")
    assert W + 3 - 1 < nt
    with pytest.raises(SlotOverwritten):
        ring_schur(L, hi, T, W, 3, ci, val, S_uu, slots=W + 3 - 2)
