"""Models of ppcsr_edge_support / ppcsr_ktruss (include/ppcsr.h), built from the partitions' exported states; numpy only.

Edge set: consumers_model.global_edges (live non-sentinel slots of every (beginning, end), slot N - 1 excluded, local src < n_p).
The undirected graph G is the upper orientation of triangles_model.upper_edges: {a, b}, a < b < n, is an edge exactly when the
pair (a, b) is stored.  support(e) is the number of triangles of G through e; truss(e) is the largest k such that e lies in a
subgraph of G whose every edge is in at least k - 2 triangles inside that subgraph (an edge in no triangle: 2; a clique on m
vertices: m).  model_truss peels synchronously: a level's threshold is the smallest remaining support, a sub-round removes every
remaining edge at or below it — this describes the graph, not a device's schedule, so its levels, sub-rounds and frontier widths
are what any synchronous sub-round peel must report."""
import numpy as np

from triangles_model import upper_edges


def triangle_list(a, b, n, chunk=1 << 22):
    """(e1, e2, e3): for every triangle x < y < z of the upper edges (a, b) (ascending by (a, b)) the indices of (x, y), (x, z),
    (y, z) — the wedge enumeration of triangles_model.model_triangles (about `chunk` wedges at a time), the closing edge found by
    a sorted-key search"""
    keys = a * n + b
    rows = np.searchsorted(a, np.arange(n + 1))
    wedges = (rows[1:] - rows[:-1])[b] if len(a) else np.zeros(0, np.int64)
    cum = np.concatenate([[0], np.cumsum(wedges)])
    out = [[np.zeros(0, np.int64)] for _ in range(3)]
    i0 = 0
    while i0 < len(a):
        i1 = min(max(int(np.searchsorted(cum, cum[i0] + chunk, side="right")) - 1, i0 + 1), len(a))
        lens = wedges[i0:i1]
        tot = int(lens.sum())
        if tot:
            e1 = np.repeat(np.arange(i0, i1), lens)
            off = np.arange(tot) - np.repeat(cum[i0:i1] - cum[i0], lens)
            e3 = rows[b[e1]] + off  # (y, z): the off-th upper edge of y
            q = a[e1] * n + b[e3]
            e2 = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
            hit = keys[e2] == q
            for o, e in zip(out, (e1, e2, e3)):
                o.append(e[hit])
        i0 = i1
    return tuple(np.concatenate(o) for o in out)


def model_support(src, dst, n):
    """(a, b, support int64[|E|], total): the edges ascending by (a, b)"""
    a, b = upper_edges(np.asarray(src), np.asarray(dst), n)
    e1, e2, e3 = triangle_list(a, b, n)
    sup = np.zeros(len(a), np.int64)
    for e in (e1, e2, e3):
        sup += np.bincount(e, minlength=len(a))
    return a, b, sup, len(e1)


def model_truss(src, dst, n):
    """dict: a, b, support, truss (int64[|E|], ascending (a, b)), total, tmax, vtruss (uint32[n]), levels, subrounds (list, per
    level), widest, first_frontier (edges) — from a synchronous sub-round peel over the triangle list"""
    a, b, sup0, total = model_support(src, dst, n)
    m = len(a)
    tri = np.stack(triangle_list(a, b, n), axis=1) if m else np.zeros((0, 3), np.int64)
    alive_t = np.ones(len(tri), bool)
    sup = sup0.copy()
    truss = np.zeros(m, np.int64)
    live = np.ones(m, bool)
    subrounds, widest, first = [], 0, 0
    # triangles of every edge: CSR over the three columns
    flat = tri.reshape(-1)
    order = np.argsort(flat, kind="stable")
    t_of = order // 3
    rows = np.searchsorted(flat[order], np.arange(m + 1))
    while live.any():
        s = int(sup[live].min())
        front = np.nonzero(live & (sup <= s))[0]
        first = first or len(front)
        here = 0
        while len(front):
            here += 1
            widest = max(widest, len(front))
            truss[front] = s + 2
            live[front] = False
            lens = rows[front + 1] - rows[front]
            idx = np.repeat(rows[front] - np.cumsum(lens) + lens, lens) + np.arange(int(lens.sum()))
            dead = np.unique(t_of[idx])
            dead = dead[alive_t[dead]]
            alive_t[dead] = False
            sup -= np.bincount(tri[dead].reshape(-1), minlength=m)
            front = np.nonzero(live & (sup <= s))[0]
        subrounds.append(here)
    vtruss = np.zeros(n, np.int64)
    np.maximum.at(vtruss, a, truss)
    np.maximum.at(vtruss, b, truss)
    return dict(a=a, b=b, support=sup0, truss=truss, total=total, tmax=int(truss.max()) if m else 0, vtruss=vtruss.astype(np.uint32),
                levels=len(subrounds), subrounds=subrounds, widest=widest, first_frontier=first)


def rows_of(a, b, value):
    """the (count, 3) uint32 rows the calls return"""
    return np.stack([a, b, value], axis=1).astype(np.uint32).reshape(-1, 3)


def counters_of(mt):
    """what ppcsr_debug_ktruss_counters [0] .. [5] must read after a ktruss call"""
    return [len(mt["a"]), mt["total"], mt["levels"], sum(mt["subrounds"]), max(mt["subrounds"], default=0), mt["widest"]]


def hardness(src, dst, n, mt, firsts=None):
    """What keeps a parity test from passing on an easy input, from the model mt = model_truss(src, dst, n) and the stored pairs.
    firsts: the partitions' first vertices, for the triangles whose three vertices do not share a partition."""
    src, dst = np.asarray(src), np.asarray(dst)
    values = np.unique(mt["truss"])
    h = dict(n=n, edges=len(mt["a"]), total=mt["total"], tmax=mt["tmax"], distinct=len(values),
             gaps=(mt["tmax"] - 1 - len(values)) if len(values) else 0,  # levels 2 .. tmax that no edge has
             levels=mt["levels"], max_subrounds=max(mt["subrounds"], default=0), widest=mt["widest"],
             first_frontier=mt["first_frontier"],
             below_support=int(np.count_nonzero(mt["truss"] < mt["support"] + 2)), max_support=int(mt["support"].max()) if len(values) else 0,
             backward=int(np.count_nonzero(src > dst)), loops=int(np.count_nonzero(src == dst)), beyond=int(np.count_nonzero(dst >= n)), cross=0)
    if firsts is not None and len(mt["a"]):
        e1, _, e3 = triangle_list(mt["a"], mt["b"], n)
        f = np.asarray(firsts, np.int64)
        part = lambda v: np.searchsorted(f, v, side="right") - 1
        h["cross"] = int(np.count_nonzero((part(mt["a"][e1]) != part(mt["b"][e1])) | (part(mt["b"][e1]) != part(mt["b"][e3]))))
    return h


def assert_hard(h, label="", **at_least):
    """every named field of hardness() is at least the given value"""
    for key, bound in at_least.items():
        assert h[key] >= bound, (label, key, bound, h)
