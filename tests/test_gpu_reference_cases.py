"""The device against the reference's own compiled code, through the public entries.

tests/golden/reference_<entry>.json hold what the reference's unmodified sources returned for the case matrix of
tests/reference_cases.py (written by tests/golden/make_reference_cases.py; tests/test_reference_pin.py holds the
oracle to the same files on the CPU).  Here cocons_cov_rns, cocons_cov_rns_classic, cocons_cov_rns_pred,
cocons_cov_rns_taper, cocons_cov_rns_taper_pred and -- on a handle created from each dense case's sites --
cocons_cov_rows must match every finite recorded entry within ENTRY_RTOL and have their non-finite entries in the
same places.  Every case runs twice with the calls in a different order and must return the same bits.  Two cases
are padded to n = 65 and n = 129 (the 64-wide pair tiles and a second factor tile are crossed); for those the
expected values are the oracle's.  Nothing outside the repository is read.
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

pytestmark = pytest.mark.gpu

ENTRY_RTOL = 2e-12      # the project's entrywise bound (tests/test_gpu_parity.py)

DEVICE_ENTRIES = [e for e in rc.ENTRIES if e != "sumsmoothlone"]
RECORDED_CASES = [(case, out) for e in DEVICE_ENTRIES for case, out in fixtures.load(e)[1]]


def assert_close(got, want, what):
    """finite entries within ENTRY_RTOL of the expected ones, non-finite ones in the same places (Inf with its sign)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN placement" % what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), "%s: Inf placement" % what
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    over = err > ENTRY_RTOL * np.abs(want[fin])
    assert not over.any(), "%s: %d of %d finite entries beyond ENTRY_RTOL, worst relative error %.3e (got %r, want %r)" % (
        what, int(over.sum()), int(fin.sum()), np.max(err[over] / np.maximum(np.abs(want[fin][over]), 1e-300)),
        got[fin][over][0], want[fin][over][0])


def full(case, recorded):
    """the recorded output in the shape the entry returns"""
    e = case["entry"]
    if e in rc.SYMMETRIC:
        n = len(case["locs"])
        S = np.zeros((n, n))
        S[np.tril_indices(n)] = recorded
        return np.where(np.tri(n, dtype=bool), S, S.T)
    if e == "cov_rns_pred":
        return recorded.reshape(len(case["locs_pred"]), len(case["locs"]))
    return recorded


def rows_of_handle(case, order):
    """cocons_cov_rows for all sites of a dense case, asked for in `order`, returned in site order"""
    import cocons_amd as ca
    th = {k: np.asarray(v, dtype=np.float64) for k, v in case["theta"].items()}
    p = th["scale"].size
    locs, X = np.asarray(case["locs"], dtype=np.float64), np.asarray(case["X"], dtype=np.float64).reshape(-1, p)
    n = locs.shape[0]
    classic = case["entry"] == "cov_rns_classic"
    fit = ca.CoconsFit(locs, X, np.arange(n, dtype=np.float64) / n, case.get("limits", [0.5, 2.5]))
    try:
        idx = np.asarray(order, dtype=np.int32)
        out = np.empty((n, n))
        out[idx] = fit.cov_rows(th, idx, classic=classic)
        return out
    finally:
        fit.close()


def device_twice(case):
    """(entry output, rows from a handle or None), computed twice with the calls in a different order and held to the
    same bits: first the one-shot entry and then the handle's rows in ascending order, then a fresh handle's rows in
    descending order followed by the one-shot entry"""
    import cocons_amd as ca
    dense = case["entry"] in rc.SYMMETRIC
    n = len(case["locs"])
    got = rc.run(case, ca)
    rows = rows_of_handle(case, np.arange(n)) if dense else None
    rows2 = rows_of_handle(case, np.arange(n)[::-1]) if dense else None
    got2 = rc.run(case, ca)
    assert rc.same_bits(got, got2), "%s: the entry's bits depend on the order of calls" % case["name"]
    if dense:
        assert rc.same_bits(rows, rows2), "%s: cocons_cov_rows' bits depend on the order of calls" % case["name"]
    return got, rows


@pytest.mark.parametrize("case,recorded", RECORDED_CASES, ids=[c["name"] for c, _ in RECORDED_CASES])
def test_device_matches_the_recorded_reference(case, recorded):
    got, rows = device_twice(case)
    want = full(case, recorded)
    assert_close(got, want, "%s (%s)" % (case["name"], case["entry"]))
    if rows is not None:
        assert_close(rows, want, "%s (cocons_cov_rows)" % case["name"])


def _by_name(name):
    return next(c for c in rc.CASES if c["name"] == name)


def _band(n, rows_m=None):
    """a band pattern of half-width 3 with the diagonal (rows_m: a rectangular one for m prediction rows)"""
    if rows_m is None:
        return rc.csr([[j for j in range(i - 3, i + 4) if 0 <= j < n] for i in range(n)])
    return rc.csr([[j for j in range(7 * i, 7 * i + 5) if j < n] for i in range(rows_m)])


def _padded_cases(n_to):
    dense = rc.padded(_by_name("rns_unequal"), n_to)
    fixed = rc.padded(_by_name("rns_fixed_1p5"), n_to)
    classic = rc.padded(_by_name("classic_base"), n_to)
    pred = dict(rc.padded(_by_name("pred_unequal"), n_to), entry="cov_rns_pred")
    ci, rp = _band(n_to)
    taper = dict(dense, entry="cov_rns_taper", colindices=ci, rowpointers=rp, name="taper_unequal_n%d" % n_to)
    pci, prp = _band(n_to, len(pred["locs_pred"]))
    tpred = dict(pred, entry="cov_rns_taper_pred", colindices=pci, rowpointers=prp, name="tpred_unequal_n%d" % n_to)
    return [dense, fixed, classic, pred, taper, tpred]


@pytest.mark.parametrize("n_to", [65, 129])
def test_device_matches_the_oracle_on_padded_cases(oracle, n_to):
    """the sites of the case matrix repeated with shifted coordinates; the oracle is held to the reference by
    tests/test_reference_pin.py"""
    for case in _padded_cases(n_to):
        got, rows = device_twice(case)
        want = rc.run(case, oracle)
        assert_close(got, want, "%s (%s)" % (case["name"], case["entry"]))
        if rows is not None:
            assert_close(rows, want, "%s (cocons_cov_rows)" % case["name"])
