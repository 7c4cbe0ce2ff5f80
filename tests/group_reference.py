"""Grouped Vecchia blocks restated in numpy and plain Python: the greedy grouping rule, the sets S of any
partition, the expanded table, the device plan and the closure check -- what cocons_amd/csrc/group_plan.hpp computes,
integer for integer.  Nothing here is floating point.

Tables are the caller's: n x m, 1-based indices of EARLIER rows, 0 = none.  Rows and blocks are 0-based inside."""
import numpy as np

ROWS_MAX = 64


def neighbours(nn, i):
    """the 0-based neighbours of row i in the order the row lists them, zeros skipped"""
    return [int(v) - 1 for v in np.asarray(nn)[i] if v > 0]


def pairs_ungrouped(nn):
    k = np.count_nonzero(np.asarray(nn).reshape(len(nn), -1) > 0, axis=1).astype(np.int64)
    return int(np.sum((k + 1) * k // 2))


def greedy(nn, max_rows=ROWS_MAX):
    """group[n]: 0-based block ids, the blocks numbered by their smallest member, ascending"""
    nn = np.asarray(nn)
    n = nn.shape[0]
    blk = list(range(n))
    S = [None] * n
    members = [[i] for i in range(n)]
    for i in range(n):
        S[i] = {i, *neighbours(nn, i)}
        for j in neighbours(nn, i):
            A, B = blk[i], blk[j]
            if A == B:
                continue
            a, b, u = len(S[A]), len(S[B]), len(S[A] | S[B])
            if u <= max_rows and u * u < a * a + b * b:
                S[A] = S[A] | S[B]
                for r in members[B]:
                    blk[r] = A
                members[A] += members[B]
                S[B], members[B] = None, None
    ids, group = {}, np.zeros(n, dtype=np.int32)
    for i in range(n):
        group[i] = ids.setdefault(blk[i], len(ids))
    return group


def plan(nn, group):
    """The plan of any partition: {"off", "rows", "mask", "order", "block", "pos", "blocks", "maxrows", "longest", "sum_rows",
    "pairs"}; blocks numbered by their smallest member whatever the labels are.  ValueError(row) when a block has |S| > 64: row
    is the 1-based smallest member of the first such block."""
    nn = np.asarray(nn)
    n = nn.shape[0]
    canon, block = {}, np.zeros(n, dtype=np.int64)
    for i in range(n):
        block[i] = canon.setdefault(int(group[i]), len(canon))
    nb = len(canon)
    mem = [[] for _ in range(nb)]
    for i in range(n):
        mem[block[i]].append(i)
    off, rows, mask, pos = [0], [], [], np.zeros(n, dtype=np.int64)
    for b in range(nb):
        s = set(mem[b])
        for i in mem[b]:
            s.update(neighbours(nn, i))
        s = sorted(s)
        if len(s) > ROWS_MAX:
            raise ValueError(mem[b][0] + 1)
        bits = 0
        for q, v in enumerate(s):
            if block[v] == b:
                bits |= 1 << q
                pos[v] = q
        rows += s
        off.append(len(rows))
        mask.append(bits)
    size = np.diff(off)
    order = sorted(range(nb), key=lambda b: (-size[b], b))
    return {"off": np.array(off), "rows": np.array(rows, dtype=np.int64), "mask": mask, "order": np.array(order, dtype=np.int64),
            "block": block, "pos": pos, "blocks": nb, "maxrows": int(size.max()) if nb else 0,
            "longest": int(pos.max()) if n else 0, "sum_rows": int(size.sum()),
            "pairs": int(np.sum(size.astype(np.int64) * (size - 1) // 2))}


def table(nn, group, m_out=None):
    """the expanded table: member i gets {s in S(block(i)) : s < i}, ascending, 1-based, zero padded to m_out columns (None: the
    longest row, at least 1)"""
    pl = plan(nn, group)
    n = len(pl["block"])
    m_out = max(pl["longest"], 1) if m_out is None else int(m_out)
    if m_out < pl["longest"]:
        raise ValueError("m_out = %d is smaller than the longest expanded row (%d)" % (m_out, pl["longest"]))
    out = np.zeros((n, m_out), dtype=np.int32, order="F")
    for i in range(n):
        o = pl["off"][pl["block"][i]]
        out[i, :pl["pos"][i]] = pl["rows"][o:o + pl["pos"][i]] + 1
    return out


def closed(nn, group):
    """0 when the table is closed under the partition (every member's row is {s in S(block) : s < i}), else the 1-based first
    row that is not; ValueError from plan() when a block has |S| > 64"""
    pl = plan(nn, group)
    nn = np.asarray(nn)
    for i in range(nn.shape[0]):
        o = pl["off"][pl["block"][i]]
        if sorted(neighbours(nn, i)) != list(pl["rows"][o:o + pl["pos"][i]]):
            return i + 1
    return 0


def table_is_valid(nn):
    """the table rules of cocons_fit_create_vecchia: 1-based indices in 1 .. row - 1 (0 = none), none twice, m <= 63"""
    nn = np.asarray(nn)
    if nn.ndim != 2 or not 1 <= nn.shape[1] <= ROWS_MAX - 1:
        return False
    for i in range(nn.shape[0]):
        v = nn[i][nn[i] != 0]
        if np.any(v < 1) or np.any(v > i) or len(set(v.tolist())) != len(v):
            return False
    return True
