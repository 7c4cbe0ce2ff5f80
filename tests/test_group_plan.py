"""The library's grouping rule, plan, expanded table and closure check (cocons_amd/csrc/group_plan.hpp, compiled into
tests/group_plan_main.cpp by the host compiler) against their numpy restatement tests/group_reference.py, integer for integer
(DESIGN.md 4y).  No GPU: the header is plain C++."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 65, 300, 641)
MS = (1, 10, 30)
CAPS = (2, 17, 64)


@functools.lru_cache(maxsize=None)
def design(n, maxmin=False):
    from cocons_amd import host
    locs = np.random.default_rng(7100 + n).uniform(0, 1, size=(n, 2))
    if maxmin:
        locs = locs[host.vecchia_order(locs).astype(np.int64) - 1]
    locs.setflags(write=False)
    return locs


@functools.lru_cache(maxsize=None)
def knn_table(n, m, maxmin=False):
    from cocons_amd import host
    nn = host.vecchia_neighbours(design(n, maxmin), m)
    nn.setflags(write=False)
    return nn


def holes_table(n, m):
    nn = knn_table(n, m).copy(order="F")
    nn[::3, m // 2] = 0
    nn[::3, 0] = 0
    nn[n // 2, :] = 0
    return nn


def star_table(n, m):
    """every row but the first names row 1 alone"""
    nn = np.zeros((n, m), dtype=np.int32, order="F")
    nn[1:, m - 1] = 1
    return nn


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/group_plan_main.cpp over cocons_amd/csrc/group_plan.hpp, by the host compiler alone (a missing compiler fails)"""
    path = str(tmp_path_factory.mktemp("group_plan") / "group_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "cocons_amd", "csrc"),
                           os.path.join(ROOT, "tests", "group_plan_main.cpp"), "-o", path])
    return path


def run(exe, path, nn, max_rows, group=None):
    nn = np.asarray(nn)
    with open(path, "w") as fh:
        fh.write("%d %d %d %d\n" % (nn.shape[0], nn.shape[1], max_rows, group is not None))
        fh.write(" ".join(map(str, nn.ravel(order="C").tolist())) + "\n")
        if group is not None:
            fh.write(" ".join(map(str, np.asarray(group).tolist())) + "\n")
    out = {}
    for line in subprocess.check_output([exe, str(path)]).decode().splitlines():
        name, *vals = line.split()
        out[name] = [int(v) for v in vals]
    return out


def check(exe, path, nn, max_rows, group=None):
    """the program's every line against the restatement; returns (labels, the restated plan)"""
    got = run(exe, path, nn, max_rows, group)
    want = GR.greedy(nn, max_rows) if group is None else np.asarray(group)
    assert got["group"] == want.tolist()
    assert got["ungrouped"] == [GR.pairs_ungrouped(nn)]
    pl = GR.plan(nn, want)
    assert got["status"] == [0]
    assert got["stats"] == [pl["blocks"], pl["maxrows"], pl["longest"], pl["sum_rows"], pl["pairs"]]
    for k in ("off", "rows", "order", "block", "pos"):
        assert got[k] == pl[k].tolist(), k
    assert got["mask"] == pl["mask"]
    assert got["table"] == GR.table(nn, want).ravel(order="C").tolist()
    assert got["closed"][0] == GR.closed(nn, want)
    assert got["expanded"] == [0, 0, 1]
    return want, pl


def structure(nn, max_rows, group, pl):
    n = nn.shape[0]
    # a partition: every row is a member of exactly one block, at one position
    members = [[pl["rows"][pl["off"][b] + q] for q in range(64) if pl["mask"][b] >> q & 1] for b in range(pl["blocks"])]
    assert sorted(v for mem in members for v in mem) == list(range(n))
    size = np.diff(pl["off"])
    assert all(pl["mask"][b] >> (int(size[b]) - 1) == 1 for b in range(pl["blocks"]))   # no bit beyond the block; the last row is a member
    # |S| <= max_rows for every block a merge made; a block of one member keeps its own rows
    for b, mem in enumerate(members):
        assert size[b] <= 64
        assert size[b] <= max_rows or len(mem) == 1
    tab = GR.table(nn, group)
    assert GR.table_is_valid(tab) and GR.closed(tab, group) == 0
    # every member conditions on a superset of its own neighbours
    for i in range(n):
        assert set(GR.neighbours(nn, i)) <= set(GR.neighbours(tab, i))
    # largest first
    assert np.all(np.diff(size[pl["order"]]) <= 0) and sorted(pl["order"].tolist()) == list(range(pl["blocks"]))


@pytest.mark.parametrize("max_rows", CAPS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_library_rule_is_the_restated_rule(n, m, max_rows, exe, tmp_path):
    nn = knn_table(n, m)
    group, pl = check(exe, tmp_path / "case.txt", nn, max_rows)
    structure(nn, max_rows, group, pl)
    if max_rows == 2:
        # nothing is merged beyond rows without neighbours: the expanded table is the input table (its rows ascending)
        tab = GR.table(nn, group, m)
        assert all(sorted(GR.neighbours(nn, i)) == GR.neighbours(tab, i) for i in range(n))


@pytest.mark.parametrize("max_rows", CAPS)
@pytest.mark.parametrize("kind", ("holes", "star", "maxmin"))
def test_holes_a_star_and_a_maxmin_design(kind, max_rows, exe, tmp_path):
    nn = {"holes": lambda: holes_table(300, 10), "star": lambda: star_table(300, 3), "maxmin": lambda: knn_table(641, 30, True)}[kind]()
    group, pl = check(exe, tmp_path / "case.txt", nn, max_rows)
    structure(nn, max_rows, group, pl)
    if kind == "star":
        # rows 1 and 2 merge (S = {0, 1} and {0}: 4 < 4 + 1); after that |S u S'| = 3 against 2 and 2, and 9 >= 8: nothing else
        assert pl["maxrows"] == 2 and pl["blocks"] == 299


def test_greedy_grouping_saves_pairs_on_a_uniform_design():
    """the plan statistics of cocons_vecchia_group at n = 641, m = 30: fewer pairs than the input table, by the rule alone"""
    nn = knn_table(641, 30)
    pl = GR.plan(nn, GR.greedy(nn, 64))
    print("vecchia-group-report cpu | pairs grouped %d ungrouped %d blocks %d" % (pl["pairs"], GR.pairs_ungrouped(nn), pl["blocks"]))
    assert pl["pairs"] < GR.pairs_ungrouped(nn)


def test_hand_made_partitions_and_labels_in_any_numbering(exe, tmp_path):
    n = 64
    every = np.zeros((n, 63), dtype=np.int32, order="F")
    for i in range(n):
        every[i, :i] = np.arange(1, i + 1)
    one = np.zeros(n, dtype=np.int32)
    group, pl = check(exe, tmp_path / "a.txt", every, 64, one)              # 64 rows, all members
    assert pl["blocks"] == 1 and pl["mask"] == [2 ** 64 - 1] and pl["pairs"] == 2016
    own = np.arange(n)[::-1].copy()                                          # labels descending: renumbered by smallest member
    group, pl = check(exe, tmp_path / "b.txt", every, 64, own)
    assert pl["blocks"] == n and pl["block"].tolist() == list(range(n)) and pl["mask"][-1] == 1 << 63
    nn = knn_table(300, 10)
    mixed = (np.arange(300) % 3).astype(np.int32)                            # |S| > 64 somewhere: refused, first block named
    got = run(exe, tmp_path / "c.txt", nn, 64, mixed)
    with pytest.raises(ValueError) as e:
        GR.plan(nn, mixed)
    assert got["status"] == [e.value.args[0]] and "stats" not in got


def test_closure_check_names_the_first_offending_row(exe, tmp_path):
    n, m = 300, 10
    nn = knn_table(n, m)
    group = GR.greedy(nn, 64)
    tab = GR.table(nn, group)
    assert GR.closed(tab, group) == 0 and run(exe, tmp_path / "ok.txt", tab, 64, group)["closed"][0] == 0
    # the input table is not closed under a grouping that merged something
    bad = GR.closed(nn, group)
    assert bad > 0 and run(exe, tmp_path / "in.txt", nn, 64, group)["closed"][0] == bad
    pl = GR.plan(tab, group)
    big = max((b for b in range(pl["blocks"]) if bin(pl["mask"][b] >> 1).count("1") >= 2), key=lambda b: pl["off"][b + 1])
    last = int(pl["rows"][pl["off"][big + 1] - 1])                           # the last row of that block: a member
    assert pl["pos"][last] >= 2
    # one neighbour too few: the row itself is named
    few = tab.copy(order="F")
    few[last, 0] = 0                                                         # (the block's first row: other members name it too)
    assert GR.closed(few, group) == last + 1
    assert run(exe, tmp_path / "few.txt", few, 64, group)["closed"] == [last + 1, pl["pos"][last] - 1, pl["pos"][last]]
    # one neighbour too many: a row outside S enlarges S, and the block's first member that lacks it is named
    outside = next(v for v in range(last) if v not in set(pl["rows"][pl["off"][big]:pl["off"][big + 1]].tolist()))
    many = np.asfortranarray(np.hstack([tab, np.zeros((n, 1), dtype=np.int32)]))
    many[last, -1] = outside + 1
    first = GR.closed(many, group)
    assert 0 < first <= last + 1 and run(exe, tmp_path / "many.txt", many, 64, group)["closed"][0] == first
    # another partition of the same rows: the block's last member moved into the block of a row nearby
    def moved(c):
        other = group.copy()
        other[last] = group[c]
        try:
            return other, GR.closed(tab, other)
        except ValueError:
            return other, -1

    other, c = next(mc for mc in (moved(c) for c in range(last - 1, 0, -1) if group[c] != group[last]) if mc[1] > 0)
    assert run(exe, tmp_path / "other.txt", tab, 64, other)["closed"][0] == c
