"""The case matrix that pins the oracle and the kernels to the reference's compiled code.

Every case is written out (no seeds): at most 12 sites, p = 1 or 3, values on a coarse binary grid so that
they print short and parse exactly.  One case = one call of one of the reference's six exports; `run`
makes that call on anything with oracle/oracle.py's signatures (the oracle, oracle/reference.py's
Reference, cocons_amd).  tests/golden/make_reference_cases.py records the reference library's outputs
for these cases; tests/test_reference_pin.py and tests/test_gpu_reference_cases.py read them back.

Which branch each case is there for (line numbers: the reference's src/cocons_full.cpp [F],
src/cocons_taper.cpp [T], src/cocons_types.h [H]):
  *_fixed_0p5/1p5/2p5   the closed forms (F:117-252, T:221-363) with smooth[0] != 0, which
                        allzeroelements (H:56-63, starts at the second element) ignores
  *_window_1p5          1.5000005 is inside mapSmoothValue's 1e-6 window (H:65-70): still case 2, but
                        with smooth_value = 1.5000005 in u
  *_quirk_0p8           equal limits outside the three windows: smooth_vector stays zero, nu = 0
  *_equal_general       equal limits but smooth[1:] != 0: the general branch at constant nu
  *_unequal             the general branch, nu varying with the covariates
  *_p1                  one column (the loop of allzeroelements never runs)
  *_706                 sites with u on both sides of 706, one of them in [700, 706), none in (708.4, 800)  (F:291-307, T:402-414)
  rns_nugget_minus_inf  nugget = -Inf (no nugget: exp(-Inf) = 0)
  rns_scale_300, rns_aniso_400   overflowing link functions: where NaN lands
The 12-site set SITES holds a coincident pair (2, 10) whose sites differ in variance and nugget, and a
pair (0, 11) that is 2^-60 apart, for which 0 < u <= eps: both take the FIRST site's diagonal value
(F:144-146 ...), the prediction variants the PREDICTION site's (F:410-414, :440-442; T:88-93, :108-111, where
the own value is sigma^2 + nugget).  The taper patterns store both pairs, have an empty row and a row that
holds only its diagonal.
"""
from __future__ import annotations

import numpy as np

INF = float("inf")
TINY = 2.0 ** -60

ENTRIES = ("cov_rns", "cov_rns_classic", "cov_rns_pred", "cov_rns_taper", "cov_rns_taper_pred", "sumsmoothlone")
SYMMETRIC = ("cov_rns", "cov_rns_classic")

# ---- sites ------------------------------------------------------------------------------------------
SITES = [[0, 0], [0.25, 0.125], [0.5, 0.75], [0.875, 0.25], [0.375, 0.625], [1, 1],
         [0.125, 0.875], [0.625, 0.375], [0.75, 0.5], [0.25, 0.5], [0.5, 0.75], [TINY, 0]]
X3 = [[1, -2, 0.5], [1, -1.5, -0.75], [1, -1, 1], [1, -0.5, -0.25], [1, 0, 0.25], [1, 0.5, -1],
      [1, 1, 0.75], [1, 1.5, -0.5], [1, 2, 0], [1, 0.25, 0.125], [1, 0.75, -0.5], [1, -1, 0.25]]
X1 = [[1]] * 12

# prediction sites: 0 coincides with observations 2 and 10, 1 is 2^-60 from observation 0, 4 coincides with 5
PRED = [[0.5, 0.75], [0, TINY], [0.3125, 0.4375], [0.9375, 0.0625], [1, 1]]
XP3 = [[1, 0.25, -0.25], [1, -0.75, 0.5], [1, 1.25, 0], [1, -1.75, 1], [1, 0.5, -1]]
XP1 = [[1]] * 5

# Range exp(-6): u = K d with K = sqrt(12 e^12) = 1397.5 at nu = 1.5.  Sites 0-4 and 5-7 are two clusters too far
# apart for anything but exp(-u) = 0.  From site 0: u = 704.2 (site 1, inside [700, 706)), 349 (2), 707.2 (3, the
# asymptotic branch).  No pair has u in (708.4, 800): there exp(-u) is subnormal or on the edge of underflow, the
# reference's own product then carries the rounding of a subnormal (relative error up to 2^-52 * 2^k after k
# lost bits, far above the entrywise bound), and no implementation can be held to its digits.
FAR = [[0, 0], [0.5, 0.0625], [0.25, 0], [0.5, 0.078125], [0.125, 0.125], [2, 2], [2.25, 2], [2.5, 2.0625]]
XF3 = X3[:8]
# the same for cov_rns_classic with smooth = (0.5, 0, 0): nu = e^0.5, K = 1465.4; from site 0: 702.1 (1), 366 (2), 706.8 (3)
FARC = [[0, 0], [0.4375, 0.1953125], [0.25, 0], [0.4375, 0.203125], [0.125, 0.125], [2, 2], [2.25, 2],
        [2.4375, 2.1953125]]
# prediction sites: 0 coincides with observation 1; 1 has u = 704.2 to observation 0, 4 has u = 707.2 to it,
# 3 has u = 704.2 to observation 5
FARP = [[0.5, 0.0625], [-0.5, -0.0625], [0.25, 0.0625], [1.5, 2.0625], [-0.5, -0.078125]]
XFP3 = XP3

# ---- patterns (1-based CSR, as spam stores them; columns ascending) ---------------------------------
TAPER_ROWS = [[0, 1, 11], [0, 1, 4, 9], [2, 4, 10], [3], [1, 2, 4, 9], [], [6, 9], [3, 7, 8], [7, 8],
              [1, 4, 6, 9], [2, 10], [0, 11]]
TPRED_ROWS = [[2, 4, 10], [0, 1, 11], [], [3, 7, 8], [5]]
FAR_ROWS = [[0, 1, 2, 3, 5], [0, 1, 3], [0, 2, 4], [0, 1, 3], [2, 4], [0, 5, 6, 7], [5, 6], [5, 7]]
FARP_ROWS = [[0, 1, 3], [0, 2, 4], [], [5, 6, 7], [0, 1]]


def csr(rows):
    """rows of 0-based column lists -> (colindices, rowpointers), both 1-based"""
    ci = [c + 1 for r in rows for c in r]
    rp = [1]
    for r in rows:
        rp.append(rp[-1] + len(r))
    return ci, rp


# ---- parameters -------------------------------------------------------------------------------------
def theta3(**over):
    th = {"std.dev": [0.25, 0.125, -0.25], "scale": [-1.5, 0.25, 0.125], "aniso": [0.25, -0.125, 0.5],
          "tilt": [0.5, 0.25, -0.25], "smooth": [0.5, 0.25, -0.5], "nugget": [-2, 0.5, 0.25]}
    th.update(over)
    return th


def theta1(**over):
    th = {"std.dev": [0.25], "scale": [-1.5], "aniso": [0.25], "tilt": [0.5], "smooth": [0.5], "nugget": [-2]}
    th.update(over)
    return th


def theta_far(**over):
    th = {"std.dev": [0.25, 0.125, -0.25], "scale": [-6, 0, 0], "aniso": [0, 0, 0], "tilt": [0, 0, 0],
          "smooth": [0, 0, 0], "nugget": [-2, 0.5, 0.25]}
    th.update(over)
    return th


FIXED = [0.75, 0, 0]      # smooth[0] != 0 and smooth[1:] == 0: "fixed" for the reference


def _smoothness_variants(prefix, entry, **common):
    """the smoothness cases every switch of the reference distinguishes, on the 12-site set"""
    out = []
    for tag, lim in (("fixed_0p5", 0.5), ("fixed_1p5", 1.5), ("fixed_2p5", 2.5), ("window_1p5", 1.5000005),
                     ("quirk_0p8", 0.8)):
        out.append(dict(name="%s_%s" % (prefix, tag), entry=entry, theta=theta3(smooth=FIXED), limits=[lim, lim], **common))
    out.append(dict(name=prefix + "_equal_general", entry=entry, theta=theta3(smooth=[0, 0.25, -0.5]),
                    limits=[1.5, 1.5], **common))
    out.append(dict(name=prefix + "_unequal", entry=entry, theta=theta3(), limits=[0.5, 2.5], **common))
    return out


def _cases():
    c = []
    dense = dict(locs=SITES, X=X3)
    # cov_rns
    c += _smoothness_variants("rns", "cov_rns", **dense)
    c.append(dict(name="rns_p1", entry="cov_rns", theta=theta1(), limits=[0.5, 2.5], locs=SITES, X=X1))
    c.append(dict(name="rns_p1_fixed_2p5", entry="cov_rns", theta=theta1(), limits=[2.5, 2.5], locs=SITES, X=X1))
    c.append(dict(name="rns_706", entry="cov_rns", theta=theta_far(), limits=[0.5, 2.5], locs=FAR, X=XF3))
    c.append(dict(name="rns_nugget_minus_inf", entry="cov_rns", theta=theta3(nugget=[-INF, 0, 0]), limits=[0.5, 2.5],
                  **dense))
    c.append(dict(name="rns_scale_300", entry="cov_rns", theta=theta3(scale=[-1.5, 300, 0.125]), limits=[0.5, 2.5],
                  **dense))
    c.append(dict(name="rns_aniso_400", entry="cov_rns", theta=theta3(aniso=[0.25, 400, 0.5]), limits=[0.5, 2.5],
                  **dense))
    # cov_rns_classic (smooth is exp(smooth' x) here, averaged over the pair)
    c.append(dict(name="classic_base", entry="cov_rns_classic", theta=theta3(), **dense))
    c.append(dict(name="classic_p1", entry="cov_rns_classic", theta=theta1(), locs=SITES, X=X1))
    c.append(dict(name="classic_706", entry="cov_rns_classic", theta=theta_far(smooth=[0.5, 0, 0]), locs=FARC, X=XF3))
    # cov_rns_pred (always the logistic smoothness, also under equal limits)
    pred = dict(locs=SITES, X=X3, locs_pred=PRED, X_pred=XP3)
    c.append(dict(name="pred_unequal", entry="cov_rns_pred", theta=theta3(), limits=[0.5, 2.5], **pred))
    c.append(dict(name="pred_equal_limits", entry="cov_rns_pred", theta=theta3(smooth=FIXED), limits=[1.5, 1.5], **pred))
    c.append(dict(name="pred_p1", entry="cov_rns_pred", theta=theta1(), limits=[0.5, 2.5], locs=SITES, X=X1,
                  locs_pred=PRED, X_pred=XP1))
    c.append(dict(name="pred_706", entry="cov_rns_pred", theta=theta_far(), limits=[0.5, 2.5], locs=FAR, X=XF3,
                  locs_pred=FARP, X_pred=XFP3))
    # cov_rns_taper
    ci, rp = csr(TAPER_ROWS)
    taper = dict(locs=SITES, X=X3, colindices=ci, rowpointers=rp)
    c += _smoothness_variants("taper", "cov_rns_taper", **taper)
    c.append(dict(name="taper_p1", entry="cov_rns_taper", theta=theta1(), limits=[0.5, 2.5], locs=SITES, X=X1,
                  colindices=ci, rowpointers=rp))
    c.append(dict(name="taper_nugget_minus_inf", entry="cov_rns_taper", theta=theta3(nugget=[-INF, 0, 0]),
                  limits=[0.5, 2.5], **taper))
    fci, frp = csr(FAR_ROWS)
    c.append(dict(name="taper_706", entry="cov_rns_taper", theta=theta_far(), limits=[0.5, 2.5], locs=FAR, X=XF3,
                  colindices=fci, rowpointers=frp))
    # cov_rns_taper_pred
    pci, prp = csr(TPRED_ROWS)
    tpred = dict(colindices=pci, rowpointers=prp, **pred)
    c.append(dict(name="tpred_unequal", entry="cov_rns_taper_pred", theta=theta3(), limits=[0.5, 2.5], **tpred))
    c.append(dict(name="tpred_equal_limits", entry="cov_rns_taper_pred", theta=theta3(smooth=FIXED), limits=[1.5, 1.5],
                  **tpred))
    c.append(dict(name="tpred_p1", entry="cov_rns_taper_pred", theta=theta1(), limits=[0.5, 2.5], locs=SITES, X=X1,
                  locs_pred=PRED, X_pred=XP1, colindices=pci, rowpointers=prp))
    fpci, fprp = csr(FARP_ROWS)
    c.append(dict(name="tpred_706", entry="cov_rns_taper_pred", theta=theta_far(), limits=[0.5, 2.5], locs=FAR, X=XF3,
                  locs_pred=FARP, X_pred=XFP3, colindices=fpci, rowpointers=fprp))
    # sumsmoothlone: both sides of |x| = 1e-4 (the bound itself is on the smoothed side), x = 0, both signs
    xs = [0.5, -0.25, 0.0001, -0.0001, 0.0001220703125, 0.00006103515625, 0, -0.00000095367431640625, 3]
    c.append(dict(name="pen_default_alpha", entry="sumsmoothlone", x=xs, lam=0.5, alpha=None))
    c.append(dict(name="pen_alpha_1e6", entry="sumsmoothlone", x=xs, lam=0.5, alpha=1e6))
    c.append(dict(name="pen_alpha_64", entry="sumsmoothlone", x=xs, lam=2, alpha=64))
    c.append(dict(name="pen_empty", entry="sumsmoothlone", x=[], lam=2, alpha=None))
    return c


CASES = _cases()
assert len({c["name"] for c in CASES}) == len(CASES)


def by_entry(entry):
    return [c for c in CASES if c["entry"] == entry]


def _a(v, cols=None):
    a = np.asarray(v, dtype=np.float64)
    return a.reshape(-1, cols) if cols else a


def run(case, impl):
    """One call of case["entry"] on `impl`.  sumsmoothlone with alpha = None is called without alpha: every
    implementation then takes its own default (the reference library the reference's default argument)."""
    e = case["entry"]
    if e == "sumsmoothlone":
        x = _a(case["x"])
        if case["alpha"] is None:
            return np.array([impl.sumsmoothlone(x, case["lam"])])
        return np.array([impl.sumsmoothlone(x, case["lam"], case["alpha"])])
    th = {k: _a(v) for k, v in case["theta"].items()}
    p = th["scale"].size
    locs, X = _a(case["locs"], 2), _a(case["X"], p)
    if e == "cov_rns":
        return impl.cov_rns(th, locs, X, case["limits"])
    if e == "cov_rns_classic":
        return impl.cov_rns_classic(th, locs, X)
    if e == "cov_rns_taper":
        return impl.cov_rns_taper(th, locs, X, case["colindices"], case["rowpointers"], case["limits"])
    lp, Xp = _a(case["locs_pred"], 2), _a(case["X_pred"], p)
    if e == "cov_rns_pred":
        return impl.cov_rns_pred(th, locs, lp, X, Xp, case["limits"])
    if e == "cov_rns_taper_pred":
        return impl.cov_rns_taper_pred(th, locs, lp, X, Xp, case["colindices"], case["rowpointers"], case["limits"])
    raise ValueError(e)


def stored(case, out):
    """what the fixtures keep of an output: the lower triangle (row-wise) where it is symmetric, else all of it
    in C order"""
    out = np.asarray(out, dtype=np.float64)
    if case["entry"] in SYMMETRIC:
        return out[np.tril_indices(out.shape[0])]
    return out.ravel()


def same_bits(a, b):
    """bit equality, NaN payloads and signs of zero included"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def padded(case, n_to):
    """`case` (a dense or taper case on observation sites) repeated with shifted coordinates up to n_to sites:
    copy k of site i sits at locs[i] + k (65 / 1024, 1 / 32), a shift no difference of two sites is a multiple of"""
    out = dict(case)
    locs, X = case["locs"], case["X"]
    n = len(locs)
    out["locs"] = [[locs[i % n][0] + 0.0634765625 * (i // n), locs[i % n][1] + 0.03125 * (i // n)] for i in range(n_to)]
    out["X"] = [list(X[i % n]) for i in range(n_to)]
    out["name"] = "%s_n%d" % (case["name"], n_to)
    return out
