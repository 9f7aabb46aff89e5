"""Models of ppcsr_kcore (include/ppcsr.h), built from the partitions' exported states.

Edge set: consumers_model.global_edges (live non-sentinel slots of every (beginning, end), slot N - 1 excluded, local src < n_p).
The undirected graph G is the upper orientation of triangles_model.upper_edges: {a, b}, a < b < n, is an edge exactly when the
pair (a, b) is stored.  model_kcore peels with the bucket queue of Batagelj and Zaversnik (2003) on Python integers; hardness
peels the same graph synchronously, level by level in sub-rounds, with numpy — an independent second route to the same core
numbers, and the source of what is asserted about an input before a parity test may count as passed."""
import numpy as np

from triangles_model import upper_edges


def symmetric_csr(src, dst, n):
    """(rows int64[n + 1], nbr int64[2 |E|]) of G: both directions of every upper edge"""
    a, b = upper_edges(np.asarray(src), np.asarray(dst), n)
    u, v = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.argsort(u, kind="stable")
    u, v = u[order], v[order]
    return np.searchsorted(u, np.arange(n + 1)), v


def model_kcore(src, dst, n):
    """core uint32[n]: Batagelj-Zaversnik — vertices kept sorted by current degree in `vert`, `start[d]` the first of degree
    d; the next vertex in order is final, and each neighbour of larger degree moves down one bucket"""
    rows, nbr = symmetric_csr(src, dst, n)
    if n == 0:
        return np.empty(0, np.uint32)
    deg = (rows[1:] - rows[:-1]).tolist()
    rows_l, nbr_l = rows.tolist(), nbr.tolist()
    md = max(deg)
    start = [0] * (md + 2)
    for d in deg:
        start[d + 1] += 1
    for d in range(1, md + 2):
        start[d] += start[d - 1]
    fill = start[:]
    vert, pos = [0] * n, [0] * n
    for v in range(n):
        pos[v] = fill[deg[v]]
        vert[pos[v]] = v
        fill[deg[v]] += 1
    for i in range(n):
        v = vert[i]
        dv = deg[v]
        for u in nbr_l[rows_l[v]:rows_l[v + 1]]:
            du = deg[u]
            if du > dv:
                pu, pw = pos[u], start[du]
                w = vert[pw]
                if u != w:
                    vert[pu], vert[pw] = w, u
                    pos[u], pos[w] = pw, pu
                start[du] += 1
                deg[u] = du - 1
    return np.array(deg, np.uint32)


def hardness(src, dst, n, core):
    """What keeps a parity test from passing on an easy input.  From a synchronous sub-round peel of the model graph: a level
    is the smallest remaining degree, a sub-round removes every remaining vertex at or below it — this describes the input,
    not a device's schedule.  The peel's own core numbers must equal `core`."""
    src, dst = np.asarray(src), np.asarray(dst)
    rows, nbr = symmetric_csr(src, dst, n)
    degree = rows[1:] - rows[:-1]
    deg = degree.copy()
    mine = np.full(n, -1, np.int64)
    levels = subrounds = max_subrounds = widest = 0
    left = n
    while left:
        k = int(deg[mine < 0].min())
        front = np.nonzero((mine < 0) & (deg <= k))[0]
        levels += 1
        here = 0
        while len(front):
            here += 1
            widest = max(widest, len(front))
            mine[front] = k
            left -= len(front)
            lens = rows[front + 1] - rows[front]
            idx = np.repeat(rows[front] - np.cumsum(lens) + lens, lens) + np.arange(int(lens.sum()))
            deg -= np.bincount(nbr[idx], minlength=n)
            front = np.nonzero((mine < 0) & (deg <= k))[0]
        subrounds += here
        max_subrounds = max(max_subrounds, here)
    assert np.array_equal(mine, np.asarray(core).astype(np.int64)), "the two peels of the model disagree"
    kmax = int(mine.max()) if n else 0
    values = np.unique(mine)
    return dict(n=n, edges=len(nbr) // 2, kmax=kmax, distinct=len(values), gaps=kmax + 1 - len(values), levels=levels, subrounds=subrounds,
                max_subrounds=max_subrounds, widest=widest, below_degree=int(np.count_nonzero(mine < degree)),
                isolated=int(np.count_nonzero(degree == 0)), maxdeg=int(degree.max()) if n else 0,
                backward=int(np.count_nonzero(src > dst)), loops=int(np.count_nonzero(src == dst)), beyond=int(np.count_nonzero(dst >= n)))


def assert_hard(h, label="", **at_least):
    """every named field of hardness() is at least the given value"""
    for key, bound in at_least.items():
        assert h[key] >= bound, (label, key, bound, h)
