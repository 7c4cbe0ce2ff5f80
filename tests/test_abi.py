"""The C-ABI shared library loads on a CPU-only machine (no HIP call at load time) and
exports every symbol include/cocons_hip.h declares.  No compute calls here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header="cocons_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cocons_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from cocons_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for nm in names:
        assert hasattr(lib, nm), "missing export " + nm
        assert nm in _lib.SIGNATURES, "python binding lacks " + nm
    assert sorted(_lib.SIGNATURES) == names
    assert lib.cocons_abi_version() == 1
    # the diagnostics live in a header of their own and are no part of the drop-in boundary
    diag = _declared("cocons_hip_diag.h")
    assert diag and not set(diag) & set(names)
    for nm in diag:
        assert hasattr(lib, nm), "missing export " + nm
    assert sorted(_lib.DIAG_SIGNATURES) == diag
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for nm in re.findall(r" T (cocons_[a-z0-9_]+)", exported):
        assert nm in names or nm in diag, "exported but declared in no header: " + nm
    # the bare-instruction probes are NOT in the product library: their own header, their own library
    probes = _declared("cocons_hip_probes.h")
    assert probes and sorted(_lib.PROBE_SIGNATURES) == probes and not set(probes) & (set(names) | set(diag))
    assert "probe" not in exported
    pl = _lib.load_probes()
    for nm in probes:
        assert hasattr(pl, nm), "missing export " + nm


def test_no_oracle_or_torch_in_product_library():
    out = subprocess.check_output(["ldd", os.path.join(ROOT, "cocons_amd", "csrc", "libcocons_hip.so")]).decode()
    assert "oracle" not in out and "torch" not in out
    assert "amdhip64" in out


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "cocons_amd")):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                src = open(os.path.join(dirpath, fn)).read()
                assert "import oracle" not in src and "from oracle" not in src and "oracle/" not in src.replace(
                    "nothing from oracle/", ""), fn


def test_host_penalty_runs_without_gpu():
    """cocons_sumsmoothlone is pure host arithmetic (src/cocons_full.cpp:12-30)."""
    import cocons_amd as ca
    assert ca.sumsmoothlone([0.5, -2.0], 2.0) == 5.0


def test_bad_arguments_return_error_codes_without_touching_the_gpu():
    """argument validation happens before any HIP call: status < 0 and a message, no abort."""
    import ctypes
    import numpy as np
    from cocons_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    a = np.zeros(8)
    p = a.ctypes.data_as(dp)
    assert lib.cocons_cov_rns(0, 1, p, p, p, p, p) < 0                             # (api_cov.hip)
    assert "bad argument" in _lib.last_error()
    assert lib.cocons_cov_rns(4, 33, p, p, p, p, p) < 0            # p > COCONS_P_MAX
    assert lib.cocons_cov_rns_pred(4, 0, 1, p, p, p, p, p, p, p) < 0
    assert lib.cocons_chol_solve(0, p, 0, None, None, None, None) < 0
    assert _lib.last_error() == "cocons_chol_solve: bad argument"                  # (api_predict.hip)
    assert not lib.cocons_fit_create(0, 1, 1, 0, p, p, p, None, p, 0)              # (api_handle.hip)
    assert lib.cocons_neg2loglik_dense(None, p, p, p, None) < 0                    # (api.hip)
    assert "null fit handle" in _lib.last_error()
    # an error raised in any translation unit of the library reaches the one cocons_last_error
    assert lib.cocons_krige_info(None, None) < 0                                   # (api_predict.hip)
    assert _lib.last_error() == "cocons_krige_info: null fit handle"
    assert lib.cocons_fisher_dense(None, p, 1, p, p, None) < 0                     # (api_grad.hip)
    assert _lib.last_error() == "cocons_fisher_dense: null fit handle"
    assert lib.cocons_multi_neg2loglik_dense(None, p, p, p, None) < 0              # (api_shard.hip)
    assert _lib.last_error() == "cocons_multi_neg2loglik_dense: null argument"
    out5 = (ctypes.c_int * 5)()
    assert lib.cocons_debug_rhs_layout(None, 0, out5) == -1           # (api_diag.hip: a diagnostic that makes no HIP call at all)
    assert _lib.last_error().startswith("cocons_debug_rhs_layout:")


def test_glue_covers_the_reference_call_surface():
    """glue/cocons_hip_glue.c (the `.Call` layer a maintainer drops into src/) defines and registers every
    native symbol of the reference's table (src/RcppExports.cpp:105-113) with the same arity, and only calls
    functions include/cocons_hip.h declares."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    glue = open(os.path.join(root, "glue", "cocons_hip_glue.c")).read()
    header = open(os.path.join(root, "include", "cocons_hip.h")).read()
    table = dict(re.findall(r'\{"(_cocons_[a-z_0-9]+)",\s*\(DL_FUNC\)&\1,\s*(\d+)\}', glue))
    reference = {"_cocons_sumsmoothlone": 3, "_cocons_cov_rns": 4, "_cocons_cov_rns_pred": 6,
                 "_cocons_cov_rns_classic": 3, "_cocons_cov_rns_taper_pred": 8, "_cocons_cov_rns_taper": 6}
    for name, arity in reference.items():
        assert int(table[name]) == arity
    for name, arity in table.items():                       # every registered symbol is defined with that arity
        m = re.search(r"^SEXP %s\(([^)]*)\)" % name, glue, re.M)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == int(arity), name
    declared = set(re.findall(r"\b(cocons_[a-z0-9_]+)\s*\(", header))
    used = set(re.findall(r"\b(cocons_[a-z0-9_]+)\s*\(", glue)) - {"cocons_hip_glue"}
    assert used <= declared, used - declared
    rfile = open(os.path.join(root, "glue", "R", "cocons_hip.R")).read()
    for sym in re.findall(r"`(_cocons_hip_[a-z_0-9]+)`", rfile):
        assert sym in table, sym


def test_glue_handle_lookup_is_sound_and_hashes_nothing():
    """The closures keep the reference's signatures (no handle argument: R/neg2loglikelihood.R:183-191), so every call looks
    its handle up.  No hashing / digest / serialisation of the data anywhere in the R glue and no package beyond base R; the
    native look-up keys on ADDRESSES, which is only sound because the keyed objects are preserved (their addresses cannot be
    recycled) and marked immutable (R code must duplicate before modifying) -- and an address hit is confirmed against the
    handle's host copies unless the glue is built with -DHIP_VERIFY_HIT=0.  (Round 4's fingerprint of 64 sampled elements let
    an R-level `z[i] <- v` through; tests/test_glue_exec.py runs that case.)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rfile = open(os.path.join(root, "glue", "R", "cocons_hip.R")).read()
    code = "\n".join(ln.split("#")[0] for ln in rfile.splitlines())
    for banned in ("hash(", "digest", "rlang::", "serialize(", "md5"):
        assert banned not in code, banned
    body = code[code.index(".cocons.hip.cached <- function"):]
    body = body[:body.index("\n}\n") + 3]
    assert "_cocons_hip_fit_cached" in body
    glue = open(os.path.join(root, "glue", "cocons_hip_glue.c")).read()
    hold = glue[glue.index("static void hip_cache_hold_keys("):]
    hold = hold[:hold.index("\n}\n")]
    assert "MARK_NOT_MUTABLE(v[k])" in hold and "R_PreserveObject(v[k])" in hold
    fn = glue[glue.index("SEXP _cocons_hip_fit_cached("):]
    hit = fn[fn.index("/* 1: the O(1) check"):fn.index("/* 2:")]
    assert "return e->handle;" in hit and "sample_sum" not in glue
    ver = hit[hit.index("#if HIP_VERIFY_HIT"):hit.index("#endif")]
    assert "cocons_fit_same_data" in ver and "hip_cache_drop(e)" in ver
    assert "cocons_fit_same_data" not in hit.replace(ver, "")        # without the option the hit touches no data
    # every path that stores an entry goes through hip_cache_hold_keys (new entry and re-key)
    assert len(re.findall(r"hip_cache_hold_keys\(e, locs, X, z,", fn)) == 2


def test_glue_compiles_against_declared_apis():
    """R is not installed here, so the glue is never linked -- but the compiler's front end can still check it: every call
    of a cocons_* entry point against include/cocons_hip.h (argument count and types) and every use of R's C API against
    the documented prototypes (tests/r_api_decls: declarations only, test infrastructure).  -Werror: an implicit
    declaration, a wrong arity or a pointer-type mismatch in a shim fails this test."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    r = subprocess.run([gcc, "-std=gnu11", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter",
                        "-Wno-cast-function-type", "-Werror", "-I", os.path.join(ROOT, "tests", "r_api_decls"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "glue", "cocons_hip_glue.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_block_ownership_deal_matches_the_python_twin():
    """cocons_shard_block_owner (no GPU call): the 256-row blocks of Sigma are dealt in groups of COCONS_SHARD_GROUP
    consecutive blocks (default 4), owner(b) = (b div G) mod world -- the same deal the gloo twin's numpy engine uses
    (tests/np_shard_engine.py)."""
    from cocons_amd import _lib
    lib = _lib.load()
    g = int(os.environ.get("COCONS_SHARD_GROUP", "4"))
    for world in (1, 2, 3, 8):
        owners = [lib.cocons_shard_block_owner(b, world) for b in range(40)]
        assert owners == [(b // g) % world for b in range(40)]
        assert all(0 <= o < world for o in owners)
    assert lib.cocons_shard_block_owner(-1, 2) == -1 and lib.cocons_shard_block_owner(0, 0) == -1


def test_debug_tune_knows_the_switch_table_and_refuses_retired_names():
    """cocons_debug_tune (no GPU call) walks the same table as the environment read: every switch of the table takes its
    default (or what the environment asked for at start-up, so the process keeps its schedule), retired switches are unknown
    names -- -1 and a message, as for any other unknown name."""
    from cocons_amd import _lib
    lib = _lib.load()
    table = {  # tune name: (environment variable or None, default)
        "engine": ("COCONS_ENGINE", 1), "dag": ("COCONS_DAG", 1), "dag_lead": ("COCONS_DAG_LEAD", 1600),
        "dag_lead2": ("COCONS_DAG_LEAD2", 600), "dag_lead3": ("COCONS_DAG_LEAD3", 1800),
        "dag_min_tiles": ("COCONS_DAG_MIN_TILES", 2000), "dag_xcc_quota": ("COCONS_DAG_XCC_QUOTA", -1),
        "dag_xcd": ("COCONS_DAG_XCD", 1), "dag_order": ("COCONS_DAG_ORDER", 1), "dag_xcd_min_quota": (None, 128),
        "dag_bw": ("COCONS_DAG_BW", 16), "dag_bh": ("COCONS_DAG_BH", 16), "dag_trace": (None, 0),
        "engine_pair": ("COCONS_ENGINE_PAIR", 1), "panel_fused": ("COCONS_PANEL_FUSED", 1),
        "potrf_follow": ("COCONS_POTRF_FOLLOW", 1), "panel_split": ("COCONS_PANEL_SPLIT", 32), "gate_sabotage": (None, 0),
        "host_delay_us": ("COCONS_DEBUG_HOST_DELAY_US", 0), "host_delay_tile": ("COCONS_DEBUG_HOST_DELAY_TILE", -1),
        "engine_in_wait_ms": (None, 0),
        "upd_waves": ("COCONS_UPD_WAVES", 8), "w8_max_tiles": ("COCONS_UPD_W8_MAX_TILES", 3500), "c_wt": (None, 0),
    }
    for name, (env, default) in table.items():
        value = int(os.environ.get(env, default)) if env else default
        assert lib.cocons_debug_tune(name.encode(), value) == 0, (name, _lib.last_error())
    for name in ("engine_block0", "panel_follow", "panel_diag", "upd_dynamic", "dag_split", "no_such_switch"):
        assert lib.cocons_debug_tune(name.encode(), 1) == -1, name
        assert _lib.last_error() == "cocons_debug_tune: unknown switch %s" % name
    assert lib.cocons_debug_tune(None, 1) == -1
