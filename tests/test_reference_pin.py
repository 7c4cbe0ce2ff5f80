"""The oracle against the reference's own compiled code (CPU only).

Live: oracle/_ref/libcocons_ref.so -- the reference's src/cocons_full.cpp, src/cocons_taper.cpp and
src/cocons_types.h compiled unmodified behind oracle/ref_wrap.cpp -- is loaded into this process next to the oracle
and must return the same BITS for every case of tests/reference_cases.py and for 50 random ones: placement and
sign of NaN, Inf and zeros included.  That is the oracle's own contract ("operation for operation"), and both
sides call the same libm and the same K_nu.  This part skips only where neither the library nor the reference's
sources exist.

Recorded: tests/golden/reference_<entry>.json hold what that library returned for the case matrix.  The oracle
is held to them within ENTRY_RTOL with non-finite entries in the same places, on every machine (pow, tgamma,
exp, cos come from the machine's libm and may differ in the last bit from the machine that wrote the files).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (HERE, os.path.join(HERE, "golden")):
    if _d not in sys.path:
        sys.path.insert(0, _d)

import reference_cases as rc                # noqa: E402
import make_reference_cases as fixtures     # noqa: E402

ENTRY_RTOL = 2e-12      # the project's entrywise bound (tests/test_gpu_parity.py)

RECORDED = {e: fixtures.load(e) for e in rc.ENTRIES}
RECORDED_CASES = [(case, out) for e in rc.ENTRIES for case, out in RECORDED[e][1]]


def _live():
    from oracle import reference
    if not reference.available():
        pytest.skip("neither oracle/_ref/libcocons_ref.so nor the reference's sources are on this machine")
    return reference.Reference()


@pytest.fixture(scope="module")
def ref(oracle):
    return _live()


def assert_same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    if not rc.same_bits(got, want):
        bad = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
        first = tuple(bad[0])
        raise AssertionError("%s: %d of %d entries differ in bits, first at %s: oracle %r (%s), reference %r (%s)"
                             % (what, len(bad), got.size, first, got[first], float(got[first]).hex(), want[first],
                                float(want[first]).hex()))


def assert_close(got, want, what):
    """finite entries within ENTRY_RTOL of the recorded ones, non-finite ones in the same places with the same sign"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN placement" % what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), "%s: Inf placement" % what
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= ENTRY_RTOL * np.abs(want[fin])), \
        "%s: max relative error %.3e" % (what, np.max(err / np.maximum(np.abs(want[fin]), 1e-300)))


# ---- live ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_oracle_is_the_reference_to_the_bit(oracle, ref, case):
    assert_same_bits(rc.run(case, oracle), rc.run(case, ref), case["name"])


def _random_case(i):
    """entry and p cycle so that every (entry, p) pair occurs; n up to 200; fixed and logistic smoothness; duplicate
    sites; one case in four with a range small enough to cross u = 706"""
    rng = np.random.default_rng(1000 + i)
    entry = rc.ENTRIES[i % 5]
    p = (1, 2, 5, 32)[i % 4]
    n = int(rng.integers(2, 201))
    m = int(rng.integers(1, 60))
    locs, lp = rng.uniform(0, 1, (n, 2)), rng.uniform(0, 1, (m, 2))
    X, Xp = rng.standard_normal((n, p)), rng.standard_normal((m, p))
    X[:, 0] = Xp[:, 0] = 1
    if n > 3:
        locs[n - 1] = locs[1]                       # coincident pair, different covariates
        lp[0] = locs[2]
    th = {k: rng.uniform(-0.3, 0.3, p) / np.sqrt(p) for k in ("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")}
    th["scale"][0] = np.log(0.003) if i % 4 == 3 else np.log(0.2)
    kind = (i // 5) % 5
    limits = [0.5, 2.5]
    if kind < 4:
        v = (0.5, 1.5, 2.5, 1.0)[kind]
        limits = [v, v]
        if rng.integers(2):
            th["smooth"][1:] = 0
    case = dict(name="random_%d" % i, entry=entry, theta=th, locs=locs, X=X, limits=limits)
    if entry in ("cov_rns_pred", "cov_rns_taper_pred"):
        case.update(locs_pred=lp, X_pred=Xp)
    if entry in ("cov_rns_taper", "cov_rns_taper_pred"):
        rows = m if entry == "cov_rns_taper_pred" else n
        pat = [sorted(set(rng.integers(0, n, int(rng.integers(0, 9))).tolist()) |
                      ({r} if entry == "cov_rns_taper" and r % 7 else set())) for r in range(rows)]
        if n > 3:
            pat[0] = sorted(set(pat[0]) | {2})       # (pred 0, obs 2) coincide; (0, 2) is an ordinary pair
            if rows > 1:
                pat[1] = sorted(set(pat[1]) | {n - 1})   # the stored coincident pair of cov_rns_taper
        case["colindices"], case["rowpointers"] = rc.csr(pat)
    return case


@pytest.mark.parametrize("i", range(50))
def test_oracle_is_the_reference_to_the_bit_on_random_cases(oracle, ref, i):
    case = _random_case(i)
    assert_same_bits(rc.run(case, oracle), rc.run(case, ref), "%s %s p=%d n=%d" % (
        case["name"], case["entry"], len(case["theta"]["scale"]), len(case["locs"])))


def test_sumsmoothlone_random(oracle, ref):
    rng = np.random.default_rng(5)
    for k in range(20):
        x = rng.standard_normal(int(rng.integers(0, 40))) * 10.0 ** rng.integers(-7, 1)
        lam = float(rng.uniform(0, 3))
        assert float(oracle.sumsmoothlone(x, lam)).hex() == float(ref.sumsmoothlone(x, lam)).hex()
        alpha = float(10.0 ** rng.integers(0, 8))
        assert float(oracle.sumsmoothlone(x, lam, alpha)).hex() == float(ref.sumsmoothlone(x, lam, alpha)).hex()


# ---- recorded --------------------------------------------------------------------------------------------------
def test_fixtures_hold_the_case_matrix():
    """the files are those of tests/reference_cases.py as it stands: same cases, same inputs"""
    def norm(c):
        return fixtures.decode_case(fixtures.encode_case(c, np.zeros((1, 1))))[0]
    assert [c["name"] for c, _ in RECORDED_CASES] == [c["name"] for c in rc.CASES]
    for (got, _), want in zip(RECORDED_CASES, rc.CASES):
        assert got == norm(want), want["name"]
    for e in rc.ENTRIES:
        assert os.path.getsize(fixtures.fixture_path(e)) <= 54 * 1024      # none larger than besselk_grid.json


@pytest.mark.parametrize("case,recorded", RECORDED_CASES, ids=[c["name"] for c, _ in RECORDED_CASES])
def test_oracle_matches_the_recorded_reference(oracle, case, recorded):
    assert_close(rc.stored(case, rc.run(case, oracle)), recorded, case["name"])


def test_recorded_reference_is_what_the_library_gives_now(ref):
    """bit for bit where the machine's libm is the one the files were written with, within ENTRY_RTOL elsewhere"""
    for e in rc.ENTRIES:
        head, cases = RECORDED[e]
        same_libm = head["libm"] == fixtures.libm_fingerprint()
        for case, recorded in cases:
            now = rc.stored(case, rc.run(case, ref))
            if same_libm:
                assert_same_bits(now, recorded, case["name"])
            else:
                assert_close(now, recorded, case["name"])
