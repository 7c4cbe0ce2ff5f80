"""tests/sequence_cases.py on the CPU: the circuits cover every ordered pair of kinds exactly once, the committed seeds give the
apply events both kinds of history, a circuit is a function of its seed, and the model of the held kriging state says what the
header says for sequences written out by hand."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sequence_cases as SC  # noqa: E402
from sequence_cases import Referee  # noqa: E402

SETS = [("dense", False), ("dense", True), ("taper", False), ("taper", True)]
sets = pytest.mark.parametrize("handle,streams", SETS)


def test_the_kinds_the_circuits_are_made_of():
    dense = {k.name: k for k in SC.DENSE_KINDS}
    taper = {k.name: k for k in SC.TAPER_KINDS}
    assert len(dense) == len(SC.DENSE_KINDS) >= 20 and len(taper) == len(SC.TAPER_KINDS) >= 14
    for kinds in (dense, taper):
        roles = Counter(k.role for k in kinds.values())
        assert roles["prepare"] == 2 and roles["prepare_fails"] == 1 and roles["release"] == 1 and roles["apply"] == 2
        assert {kinds["value_nan"].theta, kinds["value_npd"].theta} == {"nan", "npd"}
        assert kinds["prepare_a"].theta == "a" and (kinds["prepare_b_z1"].theta, kinds["prepare_b_z1"].z_col) == ("b", 1)
    assert SC.z_col_of(taper["prepare_b_z1"], 1) == 0 and SC.z_col_of(taper["prepare_b_z1"], 2) == 1


@sets
def test_circuit_covers_every_ordered_pair_once(handle, streams):
    kinds = SC.kinds_of(handle, streams)
    K = len(kinds)
    seq = SC.circuit(kinds, SC.SEEDS[handle])
    assert len(seq) == K * K + 1 and seq[0] == seq[-1]
    pairs = Counter(zip(seq[:-1], seq[1:]))
    names = [k.name for k in kinds]
    assert set(pairs) == {(a, b) for a in names for b in names}
    assert set(pairs.values()) == {1}


@sets
def test_circuit_is_a_function_of_its_seed(handle, streams):
    kinds = SC.kinds_of(handle, streams)
    assert SC.circuit(kinds, SC.SEEDS[handle]) == SC.circuit(kinds, SC.SEEDS[handle])
    assert SC.circuit(kinds, SC.SEEDS[handle]) != SC.circuit(kinds, SC.SEEDS[handle] + 1)


@sets
def test_committed_seeds_give_apply_events_both_histories(handle, streams):
    kinds = SC.kinds_of(handle, streams)
    with_state, without, count = SC.apply_shares(kinds, SC.circuit(kinds, SC.SEEDS[handle]))
    assert count == 2 * len(kinds)
    assert with_state >= SC.MIN_WITH_STATE and without >= SC.MIN_WITHOUT_STATE, (with_state, without)


@sets
@pytest.mark.parametrize("parts", [1, 2, 3, 7])
def test_split_loses_no_pair(handle, streams, parts):
    kinds = SC.kinds_of(handle, streams)
    seq = SC.circuit(kinds, SC.SEEDS[handle])
    pieces = SC.split(seq, parts)
    assert len(pieces) == parts and pieces[0][0] == seq[0] and pieces[-1][-1] == seq[-1]
    for a, b in zip(pieces[:-1], pieces[1:]):
        assert b[0] == a[-1]
    pairs = [pr for piece in pieces for pr in zip(piece[:-1], piece[1:])]
    assert pairs == list(zip(seq[:-1], seq[1:]))


@pytest.mark.parametrize("kinds", [SC.DENSE_KINDS, SC.TAPER_KINDS])
def test_model_on_sequences_written_by_hand(kinds):
    apply_, joint = [k.name for k in kinds if k.role == "apply"]
    # prepare, a failing objective, apply: the state is untouched ("No other entry point touches the state")
    m = SC.Model(kinds)
    assert m.step("prepare_a") == Referee("prepare_a", None) and m.held() == SC.Held("a", 0)
    assert m.step("value_npd") == Referee("value_npd", None)
    assert m.step("value_nan") == Referee("value_nan", None)
    assert m.step(apply_) == Referee(apply_, "prepare_a")
    assert m.step(joint) == Referee(joint, "prepare_a")
    # a second prepare replaces the first
    assert m.step("prepare_b_z1") == Referee("prepare_b_z1", None) and m.held() == SC.Held("b", 1)
    assert m.step("batch3") == Referee("batch3", None)
    assert m.step(joint) == Referee(joint, "prepare_b_z1")
    # release, apply: refused as on a fresh handle
    assert m.step("release") == Referee("release", None) and m.held() is None
    assert m.step(apply_) == Referee(apply_, None)
    # a prepare that fails leaves no state, not even the one held before
    m = SC.Model(kinds)
    m.step("prepare_a")
    assert m.step("prepare_npd") == Referee("prepare_npd", None) and m.held() is None
    assert m.step(apply_) == Referee(apply_, None)
    # a fresh handle holds none; release without a state is an event like any other
    m = SC.Model(kinds)
    assert m.step(joint) == Referee(joint, None) and m.step("release") == Referee("release", None) and m.held() is None
    # a caller's stream does not touch the state
    m = SC.Model(kinds + SC.STREAM_KINDS)
    m.step("prepare_b_z1")
    assert m.step("stream_1") == Referee("stream_1", None)
    assert m.step(apply_) == Referee(apply_, "prepare_b_z1")


def test_thetas_differ_in_every_row():
    th = SC.thetas(SC.dense_problem(130).theta)
    for row in ("mean", "std.dev", "scale", "aniso", "tilt", "smooth", "nugget"):
        assert not np.array_equal(th["a"][row], th["b"][row]), row
    assert np.isnan(th["nan"]["std.dev"][0]) and th["npd"]["std.dev"][0] == -np.inf and th["npd"]["nugget"][0] == -np.inf
    assert th["rank1"]["scale"][0] == 30.0


@pytest.mark.parametrize("n", SC.DENSE_SIZES)
def test_dense_arguments(n):
    prob, args = SC.dense_problem(n), SC.dense_args(n)
    assert prob.locs.shape == (n, 2) and prob.X.shape == (n, 3) and prob.z.shape == (n, 2) and prob.lp.shape == (70, 2)
    sizes = np.bincount(args["folds"])
    assert sizes.max() > 128 and np.sum(sizes > 128) == 1 and sizes.sum() == n and sizes.min() >= 1
    if n > 130:
        assert np.sum(sizes <= 64) >= 3          # several small folds (at n = 130 one observation is left for them)
    assert args["lp300"].shape == (300, 2) and args["dirs"].shape == (3, 6, 3)
    assert SC.dense_args(n) is args and SC.dense_problem(n) is prob


def test_dense_problem_is_the_one_of_the_sizes_tests():
    """the restated generator of tests/test_gpu_dense_sizes.problem (which also builds the oracle's matrix): same draws, same
    order -- held on the generator's state, without importing the GPU test"""
    n = 130
    rng = np.random.default_rng(6400 + n)
    locs = rng.uniform(0, 1, size=(n, 2))
    cols = [rng.standard_normal(n) * 0.5 for _ in range(2)]
    z = rng.standard_normal((n, 2))
    prob = SC.dense_problem(n)
    assert np.array_equal(prob.locs, locs) and np.array_equal(prob.X[:, 1], cols[0]) and np.array_equal(prob.z, z)
    assert np.array_equal(prob.theta["scale"], [np.log(0.2), 0.2, 0.1]) and np.array_equal(prob.theta["mean"], [0.3, -0.15, 0.2])


def test_taper_problems_are_the_smallest_of_each_layout():
    assert SC.irregular_case() == SC.IRREGULAR
    from taper_size_cases import TABLE
    assert TABLE[129][2] is False and TABLE[640][2] is True and all(not TABLE[n][2] for n in TABLE if n < 640)
    for key in SC.TAPER_PROBLEMS:
        prob, args = SC.taper_problem(key), SC.taper_args(key)
        m = prob.lp.shape[0]
        assert args["rows"].size == m - 1 and prob.special[2] not in args["rows"]
        assert len(args["uu_rows"][1]) == m and len(args["pred_rows"][1]) == m
        assert sorted(args["pivot"].tolist()) == list(range(1, prob.n + 1))
        assert set(np.unique(args["probes"]).tolist()) == {-1.0, 1.0} and args["probes"].shape == (prob.n, 8)
