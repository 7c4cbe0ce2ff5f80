"""The round rule of grouped Vecchia blocks restated in plain Python over sets: what group_rounds of
cocons_amd/csrc/group_plan.hpp and the kernels of cocons_amd/csrc/group.hip compute, integer for integer.  The candidates
are walked the way the rule states them -- the blocks of the members' neighbours --, not the way the library finds them (the
blocks of S(A)'s rows).  Nothing here is floating point.

Tables are the caller's, as in group_reference.py: n x m, 1-based indices of EARLIER rows, 0 = none."""
import numpy as np

import group_reference as GR

ROUNDS_MAX = 256


def eligible(a, b, u, max_rows):
    return u <= max_rows and u * u < a * a + b * b


def rounds(nn, max_rows=GR.ROWS_MAX, max_rounds=0):
    """(blk, S, rounds run): blk[i] the id (smallest member) of row i's block, S[id] the set of a live block (None once it is
    absorbed), and the number of rounds that merged something."""
    nn = np.asarray(nn)
    n = nn.shape[0]
    nb = [GR.neighbours(nn, i) for i in range(n)]
    blk = list(range(n))
    S = [{i, *nb[i]} for i in range(n)]
    mem = [[i] for i in range(n)]
    live = set(range(n))
    run = 0
    for _ in range(max_rounds if max_rounds > 0 else ROUNDS_MAX):
        prop = {}
        for A in live:
            a, best = len(S[A]), None
            for i in mem[A]:
                for j in nb[i]:
                    B = blk[j]
                    if B == A:
                        continue
                    b, u = len(S[B]), len(S[A] | S[B])
                    if eligible(a, b, u, max_rows):
                        k = (8192 - (a * a + b * b - u * u), B)
                        if best is None or k < best:
                            best = k
            if best is not None:
                prop[A] = best                                   # (8192 - g, B)
        if not prop:
            break
        mn = {}
        for A, (k, B) in prop.items():
            for X in (A, B):
                mn[X] = min(mn.get(X, (k, A)), (k, A))
        realised = [(A, B) for A, (k, B) in sorted(prop.items()) if mn[A] == (k, A) == mn[B]]
        touched = [X for e in realised for X in e]
        assert realised and len(set(touched)) == len(touched)    # the smallest key is realised; the edges share no block
        for A, B in realised:
            lo, hi = min(A, B), max(A, B)
            S[lo] |= S[hi]
            mem[lo] = sorted(mem[lo] + mem[hi])
            for r in mem[hi]:
                blk[r] = lo
            S[hi] = mem[hi] = None
            live.discard(hi)
        run += 1
    return blk, S, run


def labels(blk):
    """the blocks numbered by their smallest member, ascending"""
    ids, group = {}, np.zeros(len(blk), dtype=np.int32)
    for i, b in enumerate(blk):
        group[i] = ids.setdefault(b, len(ids))
    return group


def group(nn, max_rows=GR.ROWS_MAX, max_rounds=0):
    """(labels, rounds run)"""
    blk, _, run = rounds(nn, max_rows, max_rounds)
    return labels(blk), run


def open_proposals(nn, blk, S, max_rows):
    """the (A, B) with B an eligible candidate of the live block A in the state (blk, S): empty when the rule ended by itself"""
    nn = np.asarray(nn)
    out = []
    for i in range(nn.shape[0]):
        A = blk[i]
        for j in GR.neighbours(nn, i):
            B = blk[j]
            if B != A and eligible(len(S[A]), len(S[B]), len(S[A] | S[B]), max_rows):
                out.append((A, B))
    return out
