"""The round rule's entries at the boundary, without a GPU: the header declares them, the library exports them
and the ctypes bindings carry their signatures; cocons_vecchia_group_rounds answers on the host with the restatement's
integers; every call that can be refused on its arguments alone is refused with -1, the entry's name in front and the outputs
untouched -- by cocons_vecchia_group_device before any HIP call, so this machine needs no device --; the R glue registers the
shims and runs the host one against the R C-API stand-in; the host layer has the functions; the documents name them."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_reference as GR  # noqa: E402
import group_rounds_cases as GC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP = ctypes.POINTER(ctypes.c_int)
ROUNDS, DEVICE = "cocons_vecchia_group_rounds", "cocons_vecchia_group_device"


def _ip(a):
    return None if a is None else a.ctypes.data_as(IP)


def test_header_declares_binding_has_library_exports():
    from cocons_amd import _lib
    h = open(os.path.join(ROOT, "include", "cocons_hip.h")).read()
    L = _lib.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    head = r"\s*\(\s*int n,\s*int m,\s*const int \*nn,\s*int max_rows,\s*int max_rounds,\s*"
    assert re.search(r"int\s+" + ROUNDS + head + r"int \*group,\s*long long \*out5\s*\)\s*;", h)
    assert re.search(r"int\s+" + DEVICE + head + r"int device,\s*int \*group,\s*long long \*out5\s*\)\s*;", h)
    ll = ctypes.POINTER(ctypes.c_longlong)
    assert _lib.SIGNATURES[ROUNDS] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, IP, ctypes.c_int, ctypes.c_int, IP, ll])
    assert _lib.SIGNATURES[DEVICE] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, IP, ctypes.c_int, ctypes.c_int, ctypes.c_int, IP, ll])
    for entry in (ROUNDS, DEVICE):
        assert hasattr(L, entry) and re.search(r" T %s$" % entry, exported, re.M)
    assert L.cocons_abi_version() == 1


@pytest.mark.parametrize("key,max_rows,max_rounds", [((300, 10), 64, 0), ((641, 30), 64, 0), ((300, 30), 17, 0), ("lattice", 64, 0),
                                                     ("holes", 17, 0), ((641, 30), 64, 2), ((1, 1), 2, 0), ((2, 63), 64, 5)])
def test_host_entry_gives_the_restated_integers(key, max_rows, max_rounds):
    from cocons_amd import host
    nn = GC.table(key)
    want, rounds = GC.reference(key, max_rows, max_rounds)
    got, st = host.vecchia_group_rounds(nn, max_rows, max_rounds, stats=True)
    pl = GR.plan(nn, want)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert st == {"blocks": pl["blocks"], "rows": pl["sum_rows"], "pairs": pl["pairs"], "pairs_ungrouped": GR.pairs_ungrouped(nn),
                  "rounds": rounds}
    assert np.array_equal(host.vecchia_group_rounds(nn, max_rows, max_rounds), want)       # out5 = NULL


def test_refusals_without_the_gpu():
    from cocons_amd import _lib
    L = _lib.load()
    n, m = 65, 10
    nn = np.asfortranarray(GC.table((n, m)))
    group = np.full(n, 7, dtype=np.int32)
    out = (ctypes.c_longlong * 5)(*([7] * 5))
    late = nn.copy(order="F")
    late[4, 2] = 6                                   # row 5 names row 6
    twice = nn.copy(order="F")
    twice[20, 0] = twice[20, 1]
    neg = nn.copy(order="F")
    neg[9, 9] = -1
    table = "names an index outside its range (1-based indices in 1 .. row - 1, 0 = none)"
    cases = [
        (lambda f, *d: f(n, m, None, 64, 0, *d, _ip(group), out), "null argument"),
        (lambda f, *d: f(n, m, _ip(nn), 64, 0, *d, None, out), "null argument"),
        (lambda f, *d: f(0, m, _ip(nn), 64, 0, *d, _ip(group), out), "n = 0 (at least one observation expected)"),
        (lambda f, *d: f(n, 0, _ip(nn), 64, 0, *d, _ip(group), out), "m = 0 is outside 1 .. 63"),
        (lambda f, *d: f(n, 64, _ip(nn), 64, 0, *d, _ip(group), out), "m = 64 is outside 1 .. 63"),
        (lambda f, *d: f(n, m, _ip(nn), 1, 0, *d, _ip(group), out), "max_rows = 1 is outside 2 .. 64"),
        (lambda f, *d: f(n, m, _ip(nn), 65, 0, *d, _ip(group), out), "max_rows = 65 is outside 2 .. 64"),
        (lambda f, *d: f(n, m, _ip(nn), 64, -1, *d, _ip(group), out), "max_rounds = -1 (0 = 256 rounds at the most)"),
        (lambda f, *d: f(n, m, _ip(late), 64, 0, *d, _ip(group), out), "row 5 of nn " + table),
        (lambda f, *d: f(n, m, _ip(neg), 64, 0, *d, _ip(group), out), "row 10 of nn " + table),
        (lambda f, *d: f(n, m, _ip(twice), 64, 0, *d, _ip(group), out),
         "row 21 of nn names an index twice (1-based indices in 1 .. row - 1, 0 = none)"),
    ]
    for call, message in cases:
        for entry, device in ((ROUNDS, ()), (DEVICE, (0,))):
            assert call(getattr(L, entry), *device) == -1, (entry, message)
            assert _lib.last_error() == entry + ": " + message, (entry, _lib.last_error())
            assert np.all(group == 7) and list(out) == [7] * 5
    # ... and the host wrappers raise with the same text
    from cocons_amd import host
    with pytest.raises(_lib.CoconsHipError, match=ROUNDS + ": max_rows = 65"):
        host.vecchia_group_rounds(nn, 65)
    with pytest.raises(_lib.CoconsHipError, match=DEVICE + ": max_rounds = -2"):
        host.vecchia_group_device(nn, 64, -2)


def test_glue_registers_the_shims_and_runs_the_host_one():
    from test_glue_exec import RStub
    R = RStub()
    src = open(os.path.join(ROOT, "glue", "R", "cocons_hip.R")).read()
    for shim, arity, wrapper in (("_cocons_hip_vecchia_group_rounds", 3, ".cocons.hip.vecchia.group.rounds"),
                                 ("_cocons_hip_vecchia_group_device", 4, ".cocons.hip.vecchia.group.device")):
        assert R.L.stub_registered_arity(shim.encode()) == arity, shim
        body = src[src.index(wrapper + " <- function"):]
        assert "`%s`" % shim in body[:body.index("\n}\n")]
    nn = GC.table((300, 10))
    want, rounds = GC.reference((300, 10), 17)
    pl = GR.plan(nn, want)
    group, info = R.value(R.call("_cocons_hip_vecchia_group_rounds", R.real(nn.astype(float)), R.integer([17]), R.integer([0])))
    assert np.array_equal(group, want)
    assert [int(v) for v in info] == [pl["blocks"], pl["sum_rows"], pl["pairs"], GR.pairs_ungrouped(nn), rounds]
    part = R.value(R.call("_cocons_hip_vecchia_group_rounds", R.real(nn.astype(float)), R.integer([64]), R.integer([2])))
    assert np.array_equal(part[0], GC.reference((300, 10), 64, 2)[0]) and int(part[1][4]) == 2
    with pytest.raises(RuntimeError, match="cocons_vecchia_group_rounds: max_rows = 65 is outside 2 .. 64"):
        R.call("_cocons_hip_vecchia_group_rounds", R.real(nn.astype(float)), R.integer([65]), R.integer([0]))
    with pytest.raises(RuntimeError, match="cocons_vecchia_group_device: max_rounds = -1"):
        R.call("_cocons_hip_vecchia_group_device", R.real(nn.astype(float)), R.integer([64]), R.integer([-1]), R.integer([0]))
    with pytest.raises(RuntimeError, match="nn must be a matrix"):
        R.call("_cocons_hip_vecchia_group_rounds", R.real(np.zeros(5)), R.integer([64]), R.integer([0]))


def test_host_layer_has_the_functions():
    import cocons_amd as ca
    E = inspect.Parameter.empty

    def params(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]

    assert params(ca.vecchia_group_rounds) == [("nn", E), ("max_rows", 64), ("max_rounds", 0), ("stats", False)]
    assert params(ca.vecchia_group_device) == [("nn", E), ("max_rows", 64), ("max_rounds", 0), ("stats", False), ("device", 0)]
    assert params(ca.vecchia_group) == [("nn", E), ("max_rows", 64), ("stats", False)]          # pinned


def test_the_documents_name_the_entries():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"^### 4ac\. ", design, re.M)
    for entry in (ROUNDS, DEVICE, "group_rounds", "launch_group_propose"):
        assert entry in design, entry
    for entry in (ROUNDS, DEVICE):
        assert entry in readme and entry in doc, entry
    for name in (".cocons.hip.vecchia.group.rounds", ".cocons.hip.vecchia.group.device"):
        assert name in doc, name
    assert "tests/test_gpu_group_device.py" in readme
