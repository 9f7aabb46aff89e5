"""Exact host model of ppcsr_bulk_build (include/ppcsr.h): plain numpy plus the oracle's po_redistribute_positions.  It imports
nothing from the package under test, so a bulk-built state can be compared with it slot by slot (tests/bulk_checks.py).

The result of a bulk build is fully determined ("non-parity" only says it is not the layout one-by-one inserts would leave):
  1. rows with op != 0 and src < n count; num_neighbors[u] = rows with src == u, duplicates included;
  2. stable sort by (src, dst); of every run of equal keys the last row in stream order survives, with its value: E survivors;
  3. j = n + E elements; N = the smallest power of two >= N0 (the array never shrinks) with (j + 1) / N < 0.75 in fp64 (0.75 is
     the root's upper density, t_up[0] of pma_geometry.h: the root still accepts one more insert);
  4. the sequence sentinel 0, edges of vertex 0 ascending, sentinel 1, ... takes the slots po_redistribute_positions(0, N, j):
     sentinel u is element u + (survivors with src < u), the r-th survivor, of source s, is element r + s + 1;
  5. empty slots are (0xFFFFFFFF, 0, 0), sentinel u is (u, 0xFFFFFFFF, u) — value 0xFFFFFFFF for u == 0 —, an edge (src, dst, value);
  6. nodes[u] = (slot of sentinel u, slot of sentinel u + 1 or N - 1 for the last vertex, num_neighbors[u])."""
import numpy as np

from oracle_lib import oracle_lib

MAX = 0xFFFFFFFF
ROOT_UPPER_DENSITY = 0.75


def survivors(n, ops):
    """(src, dst, value of the surviving rows in (src, dst) order, num_neighbors[n]): steps 1 and 2"""
    ops = np.asarray(ops, np.uint32).reshape(-1, 3)
    kept = ops[(ops[:, 2] != 0) & (ops[:, 0] < n)]
    nn = np.bincount(kept[:, 0], minlength=n).astype(np.uint32)
    key = (kept[:, 0].astype(np.uint64) << np.uint64(32)) | kept[:, 1].astype(np.uint64)
    order = np.argsort(key, kind="stable")
    key = key[order]
    last = np.ones(len(key), bool)
    last[:-1] = key[1:] != key[:-1]
    sel = order[last]
    return kept[sel, 0], kept[sel, 1], kept[sel, 2], nn


def array_size(n, N0, E):
    """step 3"""
    N = int(N0)
    assert N > 0 and N & (N - 1) == 0, N0
    while not (float(n + E + 1) / float(N) < ROOT_UPPER_DENSITY):
        N *= 2
    return N


def bulk_model(n, N0, ops, *, lock_search=True):
    """-> (items[N, 3], nodes[n, 3]) uint32: the state ppcsr_bulk_build leaves in an empty engine of n vertices whose array holds
    N0 slots.  (lock_search does not enter the layout; it is taken so that a caller hands over the engine's whole configuration.)"""
    del lock_search
    n = int(n)
    src, dst, val, nn = survivors(n, ops)
    E = len(src)
    N = array_size(n, N0, E)
    j = n + E
    pos = np.zeros(j, np.uint64)
    oracle_lib().po_redistribute_positions(0, N, j, pos.ctypes.data)
    pos = pos.astype(np.int64)
    items = np.zeros((N, 3), np.uint32)
    items[:, 0] = MAX
    u = np.arange(n, dtype=np.int64)
    sent = pos[u + np.searchsorted(src, u, side="left")]
    items[sent, 0] = u
    items[sent, 1] = MAX
    items[sent, 2] = u
    items[sent[0], 2] = MAX
    at = pos[np.arange(E, dtype=np.int64) + src.astype(np.int64) + 1]
    items[at, 0] = src
    items[at, 1] = dst
    items[at, 2] = val
    nodes = np.empty((n, 3), np.uint32)
    nodes[:, 0] = sent
    nodes[:-1, 1] = sent[1:]
    nodes[-1, 1] = N - 1
    nodes[:, 2] = nn
    return items, nodes
