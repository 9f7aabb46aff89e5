"""Model of ppcsr_sssp / ppcsr_components, built from the partitions' exported states like tests/consumers_model.py: the
edge set is the one BFS walks (live non-sentinel slots, slot N-1 excluded, local src < n_p, dests global), with the stored
value of every edge.  Dijkstra runs on Python integers (no overflow to reason about), the components by union-find to the
smallest id.  Both results are unique, so the device is compared exactly."""
import heapq

import numpy as np

from consumers_model import NO_LEVEL

NO_PATH = 0xFFFFFFFFFFFFFFFF


def global_edges_valued(states):
    """(src, dst, value) int64 arrays of every neighbourhood edge, global ids, ascending source then slot order"""
    S, D, V = [np.empty(0, np.int64)], [np.empty(0, np.int64)], [np.empty(0, np.int64)]
    for first, items, nodes in states:
        live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)
        live[-1] = False  # slot N-1 is never part of a neighbourhood
        live &= items[:, 0] < len(nodes)
        S.append(items[live, 0].astype(np.int64) + first)
        D.append(items[live, 1].astype(np.int64))
        V.append(items[live, 2].astype(np.int64))
    src, dst, val = np.concatenate(S), np.concatenate(D), np.concatenate(V)
    order = np.argsort(src, kind="stable")
    return src[order], dst[order], val[order]


def _csr(src, dst, val, n):
    ok = dst < n  # destinations beyond the graph are skipped
    s, d, v = src[ok], dst[ok], val[ok]
    return np.searchsorted(s, np.arange(n + 1)).tolist(), d.tolist(), v.tolist()


def model_sssp(src, dst, val, n, start, with_hops=False):
    """heap Dijkstra; uint64 distances with NO_PATH.  with_hops: also the smallest number of edges among the shortest
    paths of every vertex (what a test compares with the BFS level)"""
    rows, d, v = _csr(src, dst, val, n)
    dist = [None] * n
    hops = [0] * n
    dist[start] = 0
    heap = [(0, 0, start)]
    done = [False] * n
    while heap:
        du, hu, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for i in range(rows[u], rows[u + 1]):
            x, nd = d[i], du + v[i]
            if dist[x] is None or nd < dist[x] or (nd == dist[x] and hu + 1 < hops[x] and not done[x]):
                dist[x], hops[x] = nd, hu + 1
                heapq.heappush(heap, (nd, hu + 1, x))
    out = np.array([NO_PATH if x is None else x for x in dist], np.uint64)
    return (out, np.array(hops, np.int64)) if with_hops else out


def model_components(src, dst, n):
    """union-find over the edges as undirected pairs; the label of a vertex is the smallest id of its component"""
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    ok = dst < n
    for a, b in zip(src[ok].tolist(), dst[ok].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:  # the smaller root stays a root: a root is the smallest id of its set
            if ra < rb:
                parent[rb] = ra
            else:
                parent[ra] = rb
    return np.array([find(x) for x in range(n)], np.uint32)


def levels_as_dist(levels):
    """BFS levels widened to distances (what sssp gives when every value is 1)"""
    out = levels.astype(np.uint64)
    out[levels == NO_LEVEL] = NO_PATH
    return out


def hardness(src, dst, val, n, start, levels, widest):
    """the three conditions that keep a parity test from passing on an easy input, from the model alone: the share of
    vertices reached, how many reached vertices have no shortest path as short (in edges) as their BFS level, and the widest
    BFS level against the streaming threshold"""
    dist, hops = model_sssp(src, dst, val, n, start, with_hops=True)
    reached = dist != NO_PATH
    longer = int(np.count_nonzero(reached & (hops > levels.astype(np.int64))))
    return dict(reached=int(reached.sum()), longer=longer, widest=int(widest), threshold=max(64, n // 256)), dist


def assert_hard(h, n, label=""):
    assert 4 * h["reached"] >= n, (label, h)
    assert h["longer"] >= 1, (label, h)
    assert h["widest"] >= h["threshold"], (label, h)
