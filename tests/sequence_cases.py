"""Sequences of calls on ONE fit handle (test infrastructure; numpy only, nothing of the library is imported or read).

A handle serves some twenty entries that share hidden state: the factorisation buffer whose shape changes per call, the
right-hand-side rows in slots or under the matrix, the packed band buffer of which only the envelope is cleared, the selected
inverse's second buffer, the batch slots, the held kriging state, the twin of a tapered simulation with a pivot.  The referee of
every call is the SAME call on a fresh handle: the library promises results that are repeatable to the bit, so no tolerance is
needed.  This module says which calls there are (the KINDS of events, with fixed arguments from fixed seeds), in which order
they meet (circuit: every ordered pair of kinds adjacent exactly once), and what the header promises about the one piece of
state a caller can see, the held kriging state (Model).  tests/test_sequence_cases.py holds this module on the CPU, tests/
test_gpu_sequences.py runs the circuits on the GPU.

Kinds.  A Kind is (name, role, theta, z_col):
  plain          any entry that neither reads nor writes the held kriging state
  prepare        krige_prepare / krige_taper_prepare at `theta` for realisation `z_col`: replaces the state
  prepare_fails  a prepare at a theta whose matrix is not positive definite: returns the failing minor and LEAVES NO STATE
                 (whatever was held before is gone: "It replaces any earlier state; on a non-positive pivot it returns the
                 failing minor and leaves no state")
  release        frees the state
  apply          krige_core / krige_joint_core (and the taper forms): reads the state; without one it is refused
  stream         installs a caller's stream (cocons_fit_set_stream); results behind it keep the own-stream referee
theta is one of "a", "b" (two parameter sets that differ in every row of the table and in the mean), "nan" (a NaN
parameter) and "npd" (variance and nugget exp(-inf) = 0: the zero matrix); the batch kinds take (a, bad, b).

A problem with one realisation (the envelope cases with r = 1) has no second column: its `prepare_b` takes z_col = 0 (z_col_of).
"""
from __future__ import annotations

import functools
from collections import OrderedDict, namedtuple

import numpy as np

import taper_envelope_cases as TE
import taper_size_cases as TS

Kind = namedtuple("Kind", "name role theta z_col")
Referee = namedtuple("Referee", "kind prepare")     # run `prepare` (a prepare kind's name, or None) on a fresh handle, then `kind`
Held = namedtuple("Held", "theta z_col")            # (the mean is part of the theta list)

DENSE_KINDS = (
    Kind("value_a", "plain", "a", 0),
    Kind("value_b", "plain", "b", 0),
    Kind("grad_a", "plain", "a", 0),
    Kind("profile_a", "plain", "a", 0),
    Kind("reml_b", "plain", "b", 0),
    Kind("profile_grad_b", "plain", "b", 0),
    Kind("reml_grad_a", "plain", "a", 0),
    Kind("fisher3_a", "plain", "a", 0),               # three random directions
    Kind("fisher_reml_b", "plain", "b", 0),
    Kind("cv_loo_a", "plain", "a", 0),
    Kind("cv_folds_b", "plain", "b", 0),              # one fold above 128 observations, the rest small (folds)
    Kind("batch3", "plain", "a", 0),                  # (a, rank-one matrix, b): the middle point fails
    Kind("predict70_a", "plain", "a", 0),
    Kind("predict300_b", "plain", "b", 1),            # 300 rows: the rows under the matrix grow past one tile
    Kind("prepare_a", "prepare", "a", 0),             # max_rows = 64: the 70 rows are two chunks
    Kind("prepare_b_z1", "prepare", "b", 1),
    Kind("prepare_npd", "prepare_fails", "npd", 0),
    Kind("krige70", "apply", None, 0),
    Kind("joint70", "apply", None, 0),                # covariance and three draws
    Kind("release", "release", None, 0),
    Kind("cov_rows_a", "plain", "a", 0),
    Kind("sim_b", "plain", "b", 0),
    Kind("sim_cond_a", "plain", "a", 0),
    Kind("value_nan", "plain", "nan", 0),
    Kind("value_npd", "plain", "npd", 0),
)

TAPER_KINDS = (
    Kind("value_a", "plain", "a", 0),
    Kind("value_b", "plain", "b", 0),
    Kind("grad_a", "plain", "a", 0),
    Kind("fisher_exact_a", "plain", "a", 0),          # unit probes, three directions
    Kind("fisher_probe8_b", "plain", "b", 0),         # eight random +-1 probes
    Kind("cv_a", "plain", "a", 0),
    Kind("predict_a", "plain", "a", 0),
    Kind("prepare_a", "prepare", "a", 0),             # max_rows = 64
    Kind("prepare_b_z1", "prepare", "b", 1),
    Kind("prepare_npd", "prepare_fails", "npd", 0),
    Kind("krige", "apply", None, 0),
    Kind("joint", "apply", None, 0),                  # covariance and three draws on the rows off the observations
    Kind("release", "release", None, 0),
    Kind("batch3", "plain", "a", 0),                  # (a, npd, b)
    Kind("value_nan", "plain", "nan", 0),
    Kind("value_npd", "plain", "npd", 0),
    Kind("sim_own_b", "plain", "b", 0),               # the handle's own order
    Kind("sim_pivot_a", "plain", "a", 0),             # a caller's pivot: builds (or rebuilds) the twin handle
)

STREAM_KINDS = (Kind("stream_0", "stream", None, 0), Kind("stream_1", "stream", None, 0))

# one seed per handle kind: the circuit of the kinds and the circuit of the kinds + STREAM_KINDS both meet the shares below
SEEDS = {"dense": 0, "taper": 9}
MIN_WITH_STATE, MIN_WITHOUT_STATE = 1.0 / 3.0, 1.0 / 6.0


def kinds_of(handle, streams=False):
    base = {"dense": DENSE_KINDS, "taper": TAPER_KINDS}[handle]
    return base + STREAM_KINDS if streams else base


# --------------------------------------------------------------------------- the order of the events
def circuit(kinds, seed):
    """Names of K^2 + 1 events: an Euler circuit of the complete directed graph with loops over the K kinds (Hierholzer, the
    out-edges of every kind shuffled by `seed`): every ordered pair of kinds, (k, k) included, is adjacent exactly once."""
    names = [k.name for k in kinds]
    K = len(names)
    rng = np.random.default_rng(seed)
    out = [[int(j) for j in rng.permutation(K)] for _ in range(K)]
    stack, path = [int(rng.integers(K))], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            path.append(stack.pop())
    path.reverse()
    assert len(path) == K * K + 1 and path[0] == path[-1]
    return [names[v] for v in path]


def split(seq, parts):
    """`parts` consecutive pieces of a sequence; each piece but the first BEGINS with the last event of the piece before, so that
    no adjacent pair is lost when every piece runs on a fresh handle."""
    cuts = [round(j * (len(seq) - 1) / parts) for j in range(parts + 1)]
    return [seq[cuts[j]:cuts[j + 1] + 1] for j in range(parts)]


# --------------------------------------------------------------------------- what the header promises about the held state
class Model:
    """The held kriging state of one handle as the header describes it: which prepare produced it (at which theta, z_col and
    mean), or none.  step(name) advances over one event and returns its Referee."""

    def __init__(self, kinds):
        self.kinds = OrderedDict((k.name, k) for k in kinds)
        self.state = None                      # name of the prepare kind whose state is held

    def held(self):
        if self.state is None:
            return None
        k = self.kinds[self.state]
        return Held(k.theta, k.z_col)

    def step(self, name):
        k = self.kinds[name]
        if k.role == "apply":
            return Referee(name, self.state)   # no state: refused, with the error a fresh handle gives
        if k.role == "prepare":
            self.state = name
        elif k.role in ("prepare_fails", "release"):
            self.state = None
        # plain (the failing objectives among them) and stream: "No other entry point touches the state"
        return Referee(name, None)


def referees(kinds, seq):
    """the Referee of every event of a sequence that starts on a fresh handle"""
    m = Model(kinds)
    return [m.step(name) for name in seq]


def apply_shares(kinds, seq):
    """(share of the apply events that meet a prepared state, share that meet none, number of apply events)"""
    role = {k.name: k.role for k in kinds}
    refs = [r for r in referees(kinds, seq) if role[r.kind] == "apply"]
    n_with = sum(r.prepare is not None for r in refs)
    return n_with / len(refs), (len(refs) - n_with) / len(refs), len(refs)


# --------------------------------------------------------------------------- parameters
def _copy(th):
    return OrderedDict((k, np.array(v, dtype=float)) for k, v in th.items())


def thetas(base):
    """{"a", "b", "nan", "npd", "rank1"} from a problem's theta list: b differs from a in every row of the table and in the mean;
    nan and npd as tests/test_gpu_taper_envelopes.py's _bad_thetas; rank1: range e^30, no nugget -- Sigma = s s' to rounding (the
    failing point of test_batch_matches_single_calls: a pivot fails behind the first, with tiles already written)."""
    a = _copy(base)
    b = _copy(base)
    b["mean"] = b["mean"] + np.array([0.1, -0.05, 0.05])[:b["mean"].size]
    for row, d in (("std.dev", 0.1), ("scale", 0.15), ("aniso", 0.05), ("tilt", -0.05), ("smooth", 0.1), ("nugget", 0.2)):
        b[row][0] += d
    nan = _copy(base)
    nan["std.dev"][0] = np.nan
    npd = _copy(base)
    npd["std.dev"][0] = -np.inf
    npd["nugget"][0] = -np.inf
    rank1 = _copy(base)
    for row in ("aniso", "tilt", "smooth"):
        rank1[row][:] = 0.0
    rank1["scale"][:] = 0.0
    rank1["scale"][0] = 30.0
    rank1["nugget"][:] = 0.0
    rank1["nugget"][0] = -800.0
    out = OrderedDict(a=a, b=b, nan=nan, npd=npd, rank1=rank1)
    for th in out.values():
        for v in th.values():
            v.setflags(write=False)
    return out


def z_col_of(kind, r):
    return min(kind.z_col, r - 1)


# --------------------------------------------------------------------------- dense problems and arguments
DenseProblem = namedtuple("DenseProblem", "n locs X theta z lp Xp")
DENSE_SIZES = (130, 256, 700)      # slots and front padding 126, plain | no padding, border tile rows, plain | six tiles, engine
R = 2


@functools.lru_cache(maxsize=None)
def dense_problem(n):
    """The problem of tests/test_gpu_dense_sizes.problem(n) without the oracle's matrix: the same generator, the same draws in
    the same order (p = 3, two realisations, uniform sites, 70 prediction rows)."""
    rng = np.random.default_rng(6400 + n)
    p = 3
    locs = rng.uniform(0, 1, size=(n, 2))
    X = np.asfortranarray(np.column_stack([np.ones(n)] + [rng.standard_normal(n) * 0.5 for _ in range(p - 1)]))
    th = TE.theta_full()
    th["mean"] = np.array([0.3, -0.15, 0.2])
    z = np.asfortranarray(rng.standard_normal((n, R)))
    lp = rng.uniform(0, 1, size=(70, 2))
    Xp = np.asfortranarray(np.column_stack([np.ones(70)] + [rng.standard_normal(70) * 0.5 for _ in range(p - 1)]))
    for a in (locs, X, z, lp, Xp) + tuple(th.values()):
        a.setflags(write=False)
    return DenseProblem(n, locs, X, th, z, lp, Xp)


def folds(n):
    """n labels: fold 0 holds min(n - 1, max(129, n // 2)) observations -- above the 128 a fold may have to be factored in LDS --,
    the rest go to folds of 1, 5, 30 and 64 observations in turn (at n = 130 a single observation is left for them); the
    observations are dealt in a fixed random order."""
    big = min(n - 1, max(129, n // 2))
    lab = np.zeros(n, dtype=np.int64)
    at, f, sizes = big, 1, (1, 5, 30, 64)
    while at < n:
        s = min(sizes[(f - 1) % 4], n - at)
        lab[at:at + s] = f
        at, f = at + s, f + 1
    return lab[np.random.default_rng(900 + n).permutation(n)]


@functools.lru_cache(maxsize=None)
def dense_args(n):
    """the fixed arguments of the dense kinds at size n (read-only)"""
    prob = dense_problem(n)
    rng = np.random.default_rng(77000 + n)
    p = prob.X.shape[1]
    out = dict(
        dirs=rng.standard_normal((3, 6, p)) * 0.5,
        folds=folds(n),
        lp300=rng.uniform(0, 1, size=(300, 2)),
        Xp300=np.asfortranarray(np.column_stack([np.ones(300)] + [rng.standard_normal(300) * 0.5 for _ in range(p - 1)])),
        E_joint=rng.standard_normal((70, 3)),
        E_sim=rng.standard_normal((n, 2)),
        E_cond=rng.standard_normal((70, 3)),
        rows=np.array([0, n // 2, n - 1], dtype=np.int32),
    )
    for a in out.values():
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------- taper problems and arguments
@functools.lru_cache(maxsize=None)
def irregular_case():
    """The smallest case of tests/taper_envelope_cases.py whose envelope is irregular: neither the floor alone (islands, chain)
    nor every column down to the last tile row (hub_caller).  That is lshape (n = 897; hub has 900, the clusters 1281)."""
    best = None
    for c in TE.CASES:
        prob = TE.problem(c.name)
        nt, hi, W, packed = TE.envelope_of(prob.n, prob.ref_taper[0], prob.ref_taper[1], TE.order_of(prob))
        if np.array_equal(hi, TE.floor_envelope(nt)) or np.all(hi == nt):
            continue
        if best is None or prob.n < best[0]:
            best = (prob.n, c.name)
    return best[1]


TAPER_PROBLEMS = ("n129", "n640", "irregular")      # unpacked | the first packed band buffer | an irregular envelope
IRREGULAR = "lshape"                                # == irregular_case(): held by tests/test_sequence_cases.py, not recomputed here


def taper_problem(key):
    if key == "irregular":
        return TE.problem(IRREGULAR)
    return TS.problem(int(key[1:]))


@functools.lru_cache(maxsize=None)
def taper_args(key):
    """the fixed arguments of the taper kinds of a problem (read-only): directions, probes, the joint call's rows (all but the
    row on top of an observation, where no draw is defined), their patterns, draws, a pivot"""
    prob = taper_problem(key)
    rng = np.random.default_rng(88000 + prob.n)
    p = prob.X.shape[1]
    m = prob.lp.shape[0]
    rows = np.delete(np.arange(m), prob.special[2])
    out = dict(
        dirs=rng.standard_normal((3, 6, p)) * 0.5,
        probes=np.where(rng.uniform(size=(prob.n, 8)) < 0.5, -1.0, 1.0),
        rows=rows,
        E_joint=rng.standard_normal((rows.size, 3)),
        E_sim=rng.standard_normal((prob.n, 2)),
        pivot=(rng.permutation(prob.n) + 1).astype(np.int32),
    )
    out["pred_rows"] = TE.take_rows(prob.pred_taper, rows)
    out["uu_rows"] = TE.pattern(prob.lp[rows], prob.delta)
    for a in out.values():
        for b in (a if isinstance(a, tuple) else (a,)):
            b.setflags(write=False)
    return out
