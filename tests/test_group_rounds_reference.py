"""The library's round rule (group_rounds of cocons_amd/csrc/group_plan.hpp, compiled into tests/group_rounds_main.cpp by the
host compiler -- once plainly, once with the address and undefined-behaviour sanitizers) against its restatement
tests/group_rounds_reference.py, integer for integer: labels, rounds run and plan.  Then the rule's
properties, and the theorem that a grouped model is no farther from the exact one than the table it was grouped from.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import group_rounds_cases as GC  # noqa: E402
import group_rounds_reference as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(path, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", os.path.join(ROOT, "cocons_amd", "csrc"),
                           os.path.join(ROOT, "tests", "group_rounds_main.cpp"), "-o", path])
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("group_rounds") / "group_rounds_main"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    """the same program with -fsanitize=address,undefined: a stand-alone host program, no Python inside it"""
    return _compile(str(tmp_path_factory.mktemp("group_rounds_san") / "group_rounds_main"), "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all")


def run(exe, path, nn, max_rows, max_rounds=0):
    nn = np.asarray(nn)
    with open(path, "w") as fh:
        fh.write("%d %d %d %d\n" % (nn.shape[0], nn.shape[1], max_rows, max_rounds))
        fh.write(" ".join(map(str, nn.ravel(order="C").tolist())) + "\n")
    out = {}
    res = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    for line in res.stdout.splitlines():
        name, *vals = line.split()
        out[name] = [int(v) for v in vals]
    return out


def check(exe, path, key, max_rows, max_rounds=0):
    """every line of the program against the restatement"""
    nn = GC.table(key)
    want, rounds = GC.reference(key, max_rows, max_rounds)
    got = run(exe, path, nn, max_rows, max_rounds)
    assert got["group"] == want.tolist()
    assert got["rounds"] == [rounds]
    pl = GR.plan(nn, want)
    assert got["status"] == [0]
    assert got["stats"] == [pl["blocks"], pl["maxrows"], pl["longest"], pl["sum_rows"], pl["pairs"], pl["blocks"]]
    for k in ("off", "rows", "order", "block", "pos"):
        assert got[k] == pl[k].tolist(), k
    assert got["mask"] == pl["mask"]
    assert got["table"] == GR.table(nn, want).ravel(order="C").tolist()
    return want, rounds, pl


def properties(nn, max_rows, group, pl):
    n = nn.shape[0]
    # a partition numbered by smallest member
    firsts = [int(np.flatnonzero(group == b)[0]) for b in range(pl["blocks"])]
    assert sorted(set(group.tolist())) == list(range(pl["blocks"])) and firsts == sorted(firsts)
    size = np.diff(pl["off"])
    members = np.bincount(group, minlength=pl["blocks"])
    # every block a merge made has |S| <= max_rows; a row with k + 1 > max_rows stays alone
    assert np.all((size <= max_rows) | (members == 1))
    for i in range(n):
        if len(GR.neighbours(nn, i)) + 1 > max_rows:
            assert members[group[i]] == 1
    # the expanded table is closed under the partition
    tab = GR.table(nn, group)
    assert GR.table_is_valid(tab) and GR.closed(tab, group) == 0


@pytest.mark.parametrize("max_rows", GC.CAPS)
@pytest.mark.parametrize("m", GC.MS)
@pytest.mark.parametrize("n", GC.SIZES)
def test_library_rule_is_the_restated_rule(n, m, max_rows, exe, tmp_path):
    group, rounds, pl = check(exe, tmp_path / "case.txt", (n, m), max_rows)
    properties(GC.table((n, m)), max_rows, group, pl)


@pytest.mark.parametrize("max_rows", GC.CAPS)
@pytest.mark.parametrize("kind", GC.DESIGNS)
def test_holes_star_chain_maxmin_and_lattice(kind, max_rows, exe, tmp_path):
    group, rounds, pl = check(exe, tmp_path / "case.txt", kind, max_rows)
    properties(GC.table(kind), max_rows, group, pl)
    if kind == "star":
        # every row 2 .. n proposes row 1's block with the same gain 4 + 1 - 4; the smallest id wins, S = {1, 2}; after that
        # u = 3 against 2 and 2, and 9 >= 8: one merge in one round
        assert rounds == 1 and pl["blocks"] == 299 and group[:3].tolist() == [0, 0, 1]
    if kind == "chain":
        # rows 1 and 2 merge as in the star; every other pair has u^2 = 9 >= 8
        assert rounds == 1 and pl["blocks"] == 299 and pl["maxrows"] == 2


@pytest.mark.parametrize("key,max_rows", [((641, 63), 64), ((300, 30), 17), ((641, 10), 2), ("lattice", 64), ("holes", 17), ((1, 1), 2)])
def test_sanitized_program_gives_the_same_lines(key, max_rows, exe, exe_san, tmp_path):
    nn = GC.table(key)
    assert run(exe_san, tmp_path / "san.txt", nn, max_rows) == run(exe, tmp_path / "plain.txt", nn, max_rows)
    assert run(exe_san, tmp_path / "san3.txt", nn, max_rows, 3) == run(exe, tmp_path / "plain3.txt", nn, max_rows, 3)


def test_degenerate_cases_go_one_merge_per_round():
    """m = 63 under cap 64, cap 17 under m = 30 and cap 2: a merge needs rows whose own S is small, which only the first rows
    have, and every merge raises |S| by one -- one merge per round until the cap, with the greedy rule's blocks and pairs"""
    from cocons_amd import host
    for n, m, cap, merges in ((641, 63, 64, 63), (300, 30, 17, 16), (641, 10, 2, 1)):
        nn = GC.table((n, m))
        group, rounds = GC.reference((n, m), cap)
        lib, st = host.vecchia_group_rounds(nn, cap, stats=True)                 # the library itself, not only its restatement
        assert lib.tolist() == group.tolist() and st["rounds"] == merges
        pl, greedy = GR.plan(nn, group), GR.plan(nn, GR.greedy(nn, cap))
        assert rounds == merges and pl["blocks"] == n - merges
        assert (pl["blocks"], pl["pairs"]) == (greedy["blocks"], greedy["pairs"])


@pytest.mark.parametrize("key,max_rows", [((300, 10), 64), ((300, 30), 64), ("lattice", 17), ("holes", 64)])
def test_labels_depend_on_the_neighbour_sets_alone(key, max_rows, exe, tmp_path):
    """the rows' entries permuted (zeros among them): the restatement, the stand-alone program and the library's entry all
    give the labels, the rounds and -- the program -- the plan of the table as it came"""
    from cocons_amd import host
    nn = GC.table(key)
    want, rounds = GC.reference(key, max_rows)
    rng = np.random.default_rng(5)
    mixed = np.asfortranarray(np.stack([rng.permutation(row) for row in nn]))
    assert np.any(mixed != nn)
    got, r2 = RR.group(mixed, max_rows)
    assert got.tolist() == want.tolist() and r2 == rounds
    lib, st = host.vecchia_group_rounds(mixed, max_rows, stats=True)
    assert lib.tolist() == want.tolist() and st["rounds"] == rounds
    a, b = run(exe, tmp_path / "mixed.txt", mixed, max_rows), run(exe, tmp_path / "plain.txt", nn, max_rows)
    assert a == b and a["group"] == want.tolist() and a["rounds"] == [rounds]


@pytest.mark.parametrize("key,max_rows", [((300, 10), 64), ((641, 30), 64), ("maxmin", 17), ("lattice", 64)])
def test_a_cap_on_the_rounds_stops_the_same_run_early(key, max_rows, exe, tmp_path):
    """max_rounds = t is the state after the first t rounds of the full run: the merges of round t + 1 join blocks of it"""
    nn = GC.table(key)
    full, rounds = GC.reference(key, max_rows)
    assert rounds > 3
    prev = np.arange(nn.shape[0])
    for t in (1, 2, 3):
        part, run_t = GC.reference(key, max_rows, t)
        assert run_t == t
        assert run(exe, tmp_path / ("t%d.txt" % t), nn, max_rows, t)["group"] == part.tolist()
        # a coarsening of the state before it, refined by the full run, and strictly fewer blocks every round
        for fine, coarse in ((prev, part), (part, full)):
            assert len({(a, b) for a, b in zip(fine.tolist(), coarse.tolist())}) == len(set(fine.tolist()))
        assert part.max() < prev.max()
        prev = part
    # and the state after t rounds is what a run of t rounds from the start leaves: the reference's own loop, stopped
    blk3, S3, _ = RR.rounds(nn, max_rows, 3)
    blk2, S2, _ = RR.rounds(nn, max_rows, 2)
    assert RR.labels(blk3).tolist() == GC.reference(key, max_rows, 3)[0].tolist()
    assert all(S3[b] >= S2[b] for b in set(blk3))


def _state(nn, labels):
    """(blk, S) of a partition given by labels: a block's id is its smallest member, S its members and all their neighbours"""
    first = {}
    for i, b in enumerate(np.asarray(labels).tolist()):
        first.setdefault(b, i)
    blk = [first[b] for b in np.asarray(labels).tolist()]
    S = [None] * len(blk)
    for i, A in enumerate(blk):
        S[A] = (S[A] or set()) | {i, *GR.neighbours(nn, i)}
    return blk, S


@pytest.mark.parametrize("key,max_rows", [((300, 10), 64), ((641, 30), 64), ((300, 30), 17), ("lattice", 64), ("star", 64)])
def test_a_run_that_ended_by_itself_leaves_no_eligible_candidate(key, max_rows):
    from cocons_amd import host
    nn = GC.table(key)
    blk, S, rounds = RR.rounds(nn, max_rows)
    assert rounds < RR.ROUNDS_MAX
    assert RR.open_proposals(nn, blk, S, max_rows) == []
    # the same of the LIBRARY's partition, its state rebuilt from its labels alone
    lib, st = host.vecchia_group_rounds(nn, max_rows, stats=True)
    assert st["rounds"] == rounds and RR.open_proposals(nn, *_state(nn, lib), max_rows) == []
    # ... and a capped run does leave some
    if rounds > 1:
        blk, S, _ = RR.rounds(nn, max_rows, 1)
        assert RR.open_proposals(nn, blk, S, max_rows)
        assert RR.open_proposals(nn, *_state(nn, host.vecchia_group_rounds(nn, max_rows, 1)), max_rows)


@pytest.fixture(scope="module")
def kl_setting():
    """tools/vecchia_order_kl.py's setting at n = 2500: uniform sites, an intercept-only stationary model"""
    from cocons_amd import host
    from oracle import oracle as O
    O.build()
    n = 2500
    locs = np.random.default_rng(20260000 + n).uniform(0, 1, size=(n, 2))
    th = {"mean": np.zeros(1), "std.dev": np.zeros(1), "scale": np.array([np.log(0.15)]), "aniso": np.zeros(1),
          "tilt": np.zeros(1), "smooth": np.zeros(1), "nugget": np.array([np.log(1e-8)])}
    out = {}
    for name, o in (("random", np.arange(n)), ("maxmin", host.vecchia_order(locs).astype(np.int64) - 1)):
        l = np.ascontiguousarray(locs[o])
        S = O.cov_rns(th, l, np.ones((n, 1), order="F"), (0.5, 2.5))
        out[name] = (l, S, float(np.sum(np.log(np.diag(np.linalg.cholesky(S))))))
    return out


@pytest.mark.parametrize("order", ("random", "maxmin"))
@pytest.mark.parametrize("m", (10, 30))
def test_grouped_model_is_no_farther_from_the_exact_one(m, order, kl_setting):
    """Every row of the expanded table conditions on a superset of its neighbours, so KL(grouped) <= KL(ungrouped); the
    slack is the rounding of 2500 log d in double against KL values above 0.7."""
    import knn_reference as KR
    import vecchia_reference as VR
    from cocons_amd import host
    locs, S, half_logdet = kl_setting[order]
    n = locs.shape[0]
    nn = KR.brute_self(locs, m)

    def kl(tab):
        return float(np.sum(VR.whiten(S, tab, np.zeros((n, 1)))[1])) - half_logdet

    base = kl(nn)
    line = ["ungrouped %.3f" % base]
    for name, rule in (("greedy", host.vecchia_group), ("rounds", host.vecchia_group_rounds)):
        group, st = rule(nn, 64, stats=True)
        v = kl(host.vecchia_group_table(nn, group))
        line.append("%s %.3f at %.1f pairs per obs, %d blocks" % (name, v, st["pairs"] / n, st["blocks"]))
        assert v <= base + 1e-6, (name, v, base)
    print("vecchia-group-device-report cpu | n = %d, m = %d, %s order, KL from exact: %s" % (n, m, order, "; ".join(line)))
