"""The round rule on the device (cocons_vecchia_group_device, cocons_amd/csrc/group.hip) against its
restatement tests/group_rounds_reference.py on the case list of tests/test_group_rounds_reference.py, and against the
library's own host rule (cocons_vecchia_group_rounds, pinned to the restatement at those sizes) where the restatement is too
slow.  Every comparison is of integers: labels, rounds and the statistics of the plan.  Lines "vecchia-group-device-report ..."
carry the cases (tests/golden/VECCHIA_GROUP_DEVICE_REPORT.md)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import group_rounds_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(key, max_rows, max_rounds=0):
    from cocons_amd import host
    nn = GC.table(key)
    want, rounds = GC.reference(key, max_rows, max_rounds)
    got, st = host.vecchia_group_device(nn, max_rows, max_rounds, stats=True)
    pl = GR.plan(nn, want)
    print("vecchia-group-device-report gpu | %s cap %d max_rounds %d | rounds %d (reference %d) | blocks %d (reference %d) | "
          "labels that differ %d" % (key, max_rows, max_rounds, st["rounds"], rounds, st["blocks"], pl["blocks"],
                                     int(np.count_nonzero(got != want))))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert st == {"blocks": pl["blocks"], "rows": pl["sum_rows"], "pairs": pl["pairs"], "pairs_ungrouped": GR.pairs_ungrouped(nn),
                  "rounds": rounds}
    return got, st


@pytest.mark.parametrize("max_rows", GC.CAPS)
@pytest.mark.parametrize("m", GC.MS)
@pytest.mark.parametrize("n", GC.SIZES)
def test_device_rule_is_the_restated_rule(n, m, max_rows):
    _check((n, m), max_rows)


@pytest.mark.parametrize("max_rows", GC.CAPS)
@pytest.mark.parametrize("kind", GC.DESIGNS)
def test_holes_star_chain_maxmin_and_lattice(kind, max_rows):
    _check(kind, max_rows)


def test_m63_under_cap_64_packs_the_key_at_its_extremes():
    """a = b = 64 and u = 64: the largest sizes a key is made of; one merge per round, 63 rounds"""
    _, st = _check((641, 63), 64)
    assert st["rounds"] == 63 and st["blocks"] == 641 - 63


def test_cap_17_under_m30_bars_almost_every_row():
    """every row from the 17th on has k + 1 > 17: its slot is never written and never read"""
    _, st = _check((300, 30), 17)
    assert st["rounds"] == 16 and st["blocks"] == 300 - 16


def test_many_proposers_name_one_target():
    got, st = _check("star", 64)
    assert st["rounds"] == 1 and got[:3].tolist() == [0, 0, 1]


def test_equal_gains_go_to_the_smaller_id():
    _check("lattice", 64)
    _check("lattice", 17)


@pytest.mark.parametrize("n", (1, 2))
def test_one_and_two_rows(n):
    got, st = _check((n, 1), 64)
    assert st["blocks"] == 1 and st["rounds"] == n - 1


@pytest.mark.parametrize("key,max_rows", [((641, 30), 64), ("maxmin", 64), ("lattice", 64)])
@pytest.mark.parametrize("max_rounds", (1, 3))
def test_a_cap_on_the_rounds(key, max_rows, max_rounds):
    _, st = _check(key, max_rows, max_rounds)
    assert st["rounds"] == max_rounds


def test_repeated_calls_give_the_same_integers():
    from cocons_amd import host
    nn = GC.table((641, 30))
    first = host.vecchia_group_device(nn, 64, stats=True)
    for _ in range(3):
        again = host.vecchia_group_device(nn, 64, stats=True)
        assert np.array_equal(again[0], first[0]) and again[1] == first[1]


@pytest.mark.parametrize("max_rounds", (0, 3))
def test_rounds_traced_by_events(max_rounds):
    """cocons_debug_group_rounds: the rounds recorded are the rounds launched -- one more than the rounds that merged when the
    run ends by itself, exactly max_rounds under the cap --, the live blocks fall from n to the partition's blocks"""
    import ctypes
    from cocons_amd import _lib
    L = _lib.load()
    nn = np.asfortranarray(GC.table((641, 30)))
    want, rounds = GC.reference((641, 30), 64, max_rounds)
    blocks = int(want.max()) + 1
    ip = ctypes.POINTER(ctypes.c_int)
    live, ms = np.full(64, -7, dtype=np.int32), np.full(64, -7.0)
    r = L.cocons_debug_group_rounds(641, 30, nn.ctypes.data_as(ip), 64, max_rounds, 0, 64, live.ctypes.data_as(ip), ms.ctypes.data_as(_lib.c_dp))
    assert r == (rounds + 1 if max_rounds == 0 else max_rounds), (r, rounds)
    assert live[0] == 641 and np.all(np.diff(live[:r]) <= 0) and np.all(ms[:r] > 0.0)
    assert np.all(live[r:] == -7) and np.all(ms[r:] == -7.0)
    if max_rounds == 0:
        assert live[r - 1] == blocks and live[r - 2] > blocks       # the last round starts from the final partition and finds nothing
    else:
        assert live[r - 1] > blocks                                  # the blocks BEFORE the capped run's last round
    # a record shorter than the run, and the refusals under this entry's name
    assert L.cocons_debug_group_rounds(641, 30, nn.ctypes.data_as(ip), 64, 0, 0, 2, live.ctypes.data_as(ip), ms.ctypes.data_as(_lib.c_dp)) == 2
    assert L.cocons_debug_group_rounds(641, 30, nn.ctypes.data_as(ip), 64, 0, 0, 0, live.ctypes.data_as(ip), ms.ctypes.data_as(_lib.c_dp)) == -1
    assert _lib.last_error() == "cocons_debug_group_rounds: bad argument"
    assert L.cocons_debug_group_rounds(641, 30, nn.ctypes.data_as(ip), 65, 0, 0, 8, live.ctypes.data_as(ip), ms.ctypes.data_as(_lib.c_dp)) == -1
    assert _lib.last_error() == "cocons_debug_group_rounds: max_rows = 65 is outside 2 .. 64"


def test_device_rule_is_the_host_rule_at_20000():
    """n = 20 000, m = 30, cap 64: the library's host rule is the comparator (the restatement would take minutes)"""
    from cocons_amd import host
    locs = np.random.default_rng(7100 + 20000).uniform(0, 1, size=(20000, 2))
    nn = host.vecchia_neighbours_device(locs, 30)
    want, sw = host.vecchia_group_rounds(nn, 64, stats=True)
    got, sg = host.vecchia_group_device(nn, 64, stats=True)
    print("vecchia-group-device-report gpu | n 20000 m 30 cap 64 | rounds %d | blocks %d | pairs per obs %.1f | labels that "
          "differ %d" % (sg["rounds"], sg["blocks"], sg["pairs"] / 20000.0, int(np.count_nonzero(got != want))))
    assert np.array_equal(got, want) and sg == sw
    assert sg["rounds"] > 12 and sg["pairs"] < sg["pairs_ungrouped"]


def test_refusals_that_need_a_device():
    import ctypes
    from cocons_amd import _lib
    L = _lib.load()
    nn = np.asfortranarray(GC.table((65, 10)))
    ip = ctypes.POINTER(ctypes.c_int)
    group = np.full(65, 7, dtype=np.int32)
    out = (ctypes.c_longlong * 5)(*([7] * 5))
    assert L.cocons_vecchia_group_device(65, 10, nn.ctypes.data_as(ip), 64, 0, 4096, group.ctypes.data_as(ip), out) < -100
    assert _lib.last_error().startswith("cocons_vecchia_group_device: ")
    assert np.all(group == 7) and list(out) == [7] * 5
    from cocons_amd import host
    assert np.array_equal(host.vecchia_group_device(nn, 64), GC.reference((65, 10), 64)[0])      # the next call does not find that error
    wide = np.zeros((65, 64), dtype=np.int32, order="F")
    assert L.cocons_vecchia_group_device(65, 64, wide.ctypes.data_as(ip), 64, 0, 0, group.ctypes.data_as(ip), out) == -1
    assert _lib.last_error() == "cocons_vecchia_group_device: m = 64 is outside 1 .. 63"
    assert L.cocons_vecchia_group_device(65, 0, wide.ctypes.data_as(ip), 64, 0, 0, group.ctypes.data_as(ip), out) == -1
    assert _lib.last_error() == "cocons_vecchia_group_device: m = 0 is outside 1 .. 63"
    assert np.all(group == 7) and list(out) == [7] * 5
