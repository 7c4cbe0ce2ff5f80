"""The tables the round rule is held to its restatement on, and that restatement's answers, computed once
per session and shared by tests/test_group_rounds_reference.py (the host rule) and tests/test_gpu_group_device.py (the device
rule).  Not a test module.  Tables are the caller's: n x m int32 in Fortran order, 1-based, 0 = none, read-only."""
import functools

import numpy as np

import group_rounds_reference as RR

SIZES = (1, 2, 65, 300, 641)
MS = (1, 10, 30, 63)
CAPS = (2, 17, 64)
DESIGNS = ("holes", "star", "chain", "maxmin", "lattice")


@functools.lru_cache(maxsize=None)
def knn_table(n, m, maxmin=False):
    from cocons_amd import host
    locs = np.random.default_rng(7100 + n).uniform(0, 1, size=(n, 2))
    if maxmin:
        locs = locs[host.vecchia_order(locs).astype(np.int64) - 1]
    nn = host.vecchia_neighbours(locs, m)
    nn.setflags(write=False)
    return nn


@functools.lru_cache(maxsize=None)
def design_table(kind):
    from cocons_amd import host
    if kind == "holes":
        nn = knn_table(300, 10).copy(order="F")
        nn[::3, 5] = 0
        nn[::3, 0] = 0
        nn[150, :] = 0
    elif kind == "star":                     # every row but the first names row 1 alone: 299 proposers, one target
        nn = np.zeros((300, 3), dtype=np.int32, order="F")
        nn[1:, 2] = 1
    elif kind == "chain":                    # row i names row i - 1
        nn = np.zeros((300, 2), dtype=np.int32, order="F")
        nn[1:, 0] = np.arange(1, 300)
    elif kind == "maxmin":
        nn = knn_table(641, 30, True).copy(order="F")
    elif kind == "lattice":                  # a 20 x 20 lattice with exact coordinates, row by row: many equal gains
        gy, gx = np.divmod(np.arange(400), 20)
        nn = host.vecchia_neighbours(np.column_stack([gx, gy]).astype(np.float64), 10)
    else:
        raise KeyError(kind)
    nn.setflags(write=False)
    return nn


@functools.lru_cache(maxsize=None)
def reference(key, max_rows, max_rounds=0):
    """(labels, rounds run) of the restated rule; key: (n, m) of knn_table, or a design's name"""
    nn = design_table(key) if isinstance(key, str) else knn_table(*key)
    group, run = RR.group(nn, max_rows, max_rounds)
    group.setflags(write=False)
    return group, run


def table(key):
    return design_table(key) if isinstance(key, str) else knn_table(*key)
