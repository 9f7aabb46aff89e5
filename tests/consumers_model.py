"""numpy model of the reference's consumer templates (src/utility/bfs.h:15-36, src/utility/pagerank.h:15-29) instantiated
with T = PPPCSR, built from the partitions' exported states: get_neighbourhood(s) routed to the owner of s (PPPCSR.cpp:76-80)
= the live slots of (beginning, end) of its local id, dests as stored (global); getNode(s).num_neighbors likewise."""
import numpy as np

NO_LEVEL = 0xFFFFFFFF


def partition_states(pp):
    """[(first global vertex, items, nodes)] of every partition of a PPPCSR, in partition order"""
    out = []
    for k in range(pp.num_partitions()):
        items, nodes = pp.partition(k).state()
        out.append((int(pp.partition_start(k)), items, nodes))
    return out


def last_slot_free(items):
    """slot N-1 belongs to no neighbourhood: an edge there would be left out by one layout and not by another"""
    v = items[-1]
    return not (v[2] != 0 and v[1] != 0xFFFFFFFF and v[2] != 0xFFFFFFFF)


def global_edges(states):
    """(src, dst) int64 arrays of every neighbourhood edge, global ids, in the templates' order: ascending global source,
    then slot order"""
    S, D = [np.empty(0, np.int64)], [np.empty(0, np.int64)]
    for first, items, nodes in states:
        live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)
        live[-1] = False  # slot N-1 is never part of a neighbourhood
        live &= items[:, 0] < len(nodes)
        S.append(items[live, 0].astype(np.int64) + first)
        D.append(items[live, 1].astype(np.int64))
    src, dst = np.concatenate(S), np.concatenate(D)
    order = np.argsort(src, kind="stable")
    return src[order], dst[order]


def num_neighbors(states):
    return np.concatenate([nodes[:, 2] for _, _, nodes in states]) if states else np.empty(0, np.uint32)


def model_bfs(src, dst, n, start):
    """bfs.h: levels of a queue walk from `start` (levels are unique, so a level-by-level walk gives the same)"""
    lv = np.full(n, NO_LEVEL, np.uint32)
    lv[start] = 0
    ok = dst < n  # (the template would index out of bounds)
    s, d = src[ok], dst[ok]
    rows = np.searchsorted(s, np.arange(n + 1))
    front = np.array([start], np.int64)
    level = 0
    widest = 1
    while len(front):
        a, lens = rows[front], rows[front + 1] - rows[front]
        idx = np.repeat(a - np.cumsum(lens) + lens, lens) + np.arange(int(lens.sum()))
        nb = d[idx]
        nb = np.unique(nb[lv[nb] == NO_LEVEL])
        level += 1
        lv[nb] = level
        front = nb
        widest = max(widest, len(front))
    return lv, widest


def model_pagerank(src, dst, nn, node_values):
    """pagerank.h: out[d] += node_values[s] / num_neighbors(s), fp32, edges in ascending source order (np.add.at applies
    its updates one at a time in index order)"""
    n = len(nn)
    vals = np.asarray(node_values, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        contrib = (vals / nn.astype(np.float32)).astype(np.float32)
    out = np.zeros(n, np.float32)
    ok = dst < n
    np.add.at(out, dst[ok], contrib[src[ok]])
    return out
