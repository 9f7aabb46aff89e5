"""Model of ppcsr_msf / pppcsr_msf: numpy and Python integers only, nothing of the package.  Built from the partitions' exported
states through paths_model.global_edges_valued: every stored pair (a, b), a != b, b < n, with value w is an undirected edge of
key (w, lo, hi); equal keys (the two directions of a pair stored with equal values) count once.  Under that strict order the
minimum spanning forest is unique, so the device is compared exactly.  model_msf is Kruskal's algorithm with union-find;
model_rounds is a synchronous replica of the device's Boruvka schedule, which must choose the same keys."""
import numpy as np

from paths_model import model_components


def edge_keys(src, dst, val, n):
    """the distinct keys as int64 columns (w, lo, hi), in ascending key order"""
    src, dst, val = (np.asarray(x, np.int64) for x in (src, dst, val))
    ok = (dst < n) & (src != dst)
    lo, hi, w = np.minimum(src[ok], dst[ok]), np.maximum(src[ok], dst[ok]), val[ok]
    order = np.lexsort((hi, lo, w))
    w, lo, hi = w[order], lo[order], hi[order]
    keep = np.ones(len(w), bool)
    keep[1:] = (w[1:] != w[:-1]) | (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    return w[keep], lo[keep], hi[keep]


def model_msf(src, dst, val, n):
    """(edges int64[count, 3] rows (lo, hi, w) ascending by (lo, hi), weight as a Python int, labels uint32): Kruskal in key
    order; labels from model_components"""
    w, lo, hi = edge_keys(src, dst, val, n)
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    picked = []
    for i, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            picked.append(i)
    picked = np.array(picked, np.int64)
    edges = np.stack([lo[picked], hi[picked], w[picked]], axis=1).reshape(-1, 3)
    edges = edges[np.lexsort((edges[:, 1], edges[:, 0]))]
    weight = sum(int(x) for x in edges[:, 2].tolist())
    return edges, weight, model_components(np.asarray(src, np.int64), np.asarray(dst, np.int64), n)


def _depths(parent):
    """the number of links from every vertex to its root, by pointer doubling"""
    ptr = parent.copy()
    dist = (ptr != np.arange(len(ptr))).astype(np.int64)
    while True:
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            return dist
        dist = dist + dist[ptr]
        ptr = nxt


def model_rounds(src, dst, val, n, with_detail=False):
    """A synchronous replica of the schedule.  Per round: every component's smallest cut key; every component with one hooks
    to the component at the key's other end, except that of a mutual pair (two components that chose one key) the smaller id
    stays a root.  Returns (hooks per round, deepest parent chain per round) over the hooking rounds — the device makes one
    more round, which finds no cut edge.  with_detail: also the chosen keys as a set of (w, lo, hi) and the number of choices
    in which another cut key of the component had the chosen weight."""
    w, lo, hi = edge_keys(src, dst, val, n)
    rank = np.arange(len(w), dtype=np.int64)  # keys are sorted: the rank IS the order
    comp = np.arange(n, dtype=np.int64)
    none = len(w)
    hooks, depth, chosen, ties = [], [], set(), 0
    while True:
        ca, cb = comp[lo], comp[hi]
        cut = ca != cb
        if not cut.any():
            break
        best = np.full(n, none, np.int64)
        np.minimum.at(best, ca[cut], rank[cut])
        np.minimum.at(best, cb[cut], rank[cut])
        roots = np.nonzero(best < none)[0]
        k = best[roots]
        other = np.where(ca[k] == roots, cb[k], ca[k])
        mutual = best[other] == k
        stays = mutual & (roots < other)
        parent = comp.copy()  # (comp[v] is v's root: a compressed parent array)
        parent[roots[~stays]] = other[~stays]
        hooks.append(int((~stays).sum()))
        depth.append(int(_depths(parent).max()))
        chosen.update(zip(w[k].tolist(), lo[k].tolist(), hi[k].tolist()))
        if with_detail:
            same = np.zeros(n, np.int64)  # cut keys of the chosen weight, per component
            np.add.at(same, ca[cut], (w[cut] == w[best[ca[cut]]]).astype(np.int64))
            np.add.at(same, cb[cut], (w[cut] == w[best[cb[cut]]]).astype(np.int64))
            ties += int((same[roots] >= 2).sum())
        ptr = parent
        while True:
            nxt = ptr[ptr]
            if np.array_equal(nxt, ptr):
                break
            ptr = nxt
        comp = ptr
    return (hooks, depth, chosen, ties) if with_detail else (hooks, depth)


def hardness(src, dst, val, n, edges=None):
    """conditions on the input, from the model alone, that keep a parity test from passing on an easy input"""
    src, dst, val = (np.asarray(x, np.int64) for x in (src, dst, val))
    if edges is None:
        edges = model_msf(src, dst, val, n)[0]
    hooks, depth, chosen, ties = model_rounds(src, dst, val, n, with_detail=True)
    forest = set(zip(edges[:, 2].tolist(), edges[:, 0].tolist(), edges[:, 1].tolist()))
    assert forest == chosen, "Boruvka's keys differ from Kruskal's"
    stored = {(a, b): v for a, b, v in zip(src.tolist(), dst.tolist(), val.tolist())}
    opposite = reverse_only = 0
    for (wt, a, b) in forest:
        f, r = stored.get((a, b)), stored.get((b, a))
        if f is not None and r is not None and f != r and wt == min(f, r):
            opposite += 1
        if f is None and r == wt:
            reverse_only += 1
    touched = np.zeros(n, bool)
    ok = (dst < n) & (src != dst)
    touched[src[ok]] = True
    touched[dst[ok]] = True
    labels = model_components(src, dst, n)
    sizes = np.bincount(labels, minlength=n)
    return dict(ties=ties, opposite=opposite, reverse_only=reverse_only, loops=int((src == dst).sum()), beyond=int((dst >= n).sum()),
                isolated=int((~touched).sum()), trees=int((sizes > 1).sum()), rounds=len(hooks), hooks=hooks, depth=depth)


HARD = dict(ties=1, opposite=1, reverse_only=1, loops=1, beyond=1, isolated=1, trees=2, rounds=3)


def assert_hard(h, label, **floors):
    """every key of floors is a lower bound on h[key]"""
    for key, least in floors.items():
        assert h[key] >= least, f"{label}: the input is too easy: {key} = {h[key]} < {least} ({h})"


def zoo(streams, n, scale, core_edges, seed):
    """adds (uint32 rows src, dst, value) over n vertices: a folded RMAT core with values in [1, 4]; a block of 64 ids with 150
    pairs of one value (only (lo, hi) breaks their ties); opposite pairs with different values, the lighter one forward or
    backward; a ruler path on 32 ids that nothing else touches (rounds); values 1 and 2^32 - 2; self-loops; destinations beyond n"""
    rng = np.random.default_rng(seed)
    s, d = streams.rmat_edges_folded(n, scale, core_edges, seed=seed)
    rows = [np.stack([s, d, rng.integers(1, 5, len(s))], axis=1).astype(np.int64)]
    b0 = n // 2
    rows.append(np.stack([b0 + rng.integers(0, 64, 150), b0 + rng.integers(0, 64, 150), np.full(150, 9)], axis=1))
    a, b = rng.integers(0, n, 60), rng.integers(0, n, 60)
    light, heavy = rng.integers(1, 3, 60), rng.integers(3, 7, 60)
    fwd = rng.integers(0, 2, 60).astype(bool)
    rows.append(np.stack([a, b, np.where(fwd, light, heavy)], axis=1))
    rows.append(np.stack([b, a, np.where(fwd, heavy, light)], axis=1))
    ext = rng.integers(0, n, (12, 2))
    rows.append(np.stack([ext[:, 0], ext[:, 1], np.where(np.arange(12) % 2 == 0, 1, 0xFFFFFFFE)], axis=1))
    loops = rng.integers(0, n, 6)
    rows.append(np.stack([loops, loops, np.full(6, 2)], axis=1))
    rows.append(np.stack([rng.integers(0, n, 6), n + rng.integers(0, 9, 6), np.full(6, 1)], axis=1))
    # the ruler path on 32 ids that nothing above touches: a tree of its own that takes exactly 5 hooking rounds
    rest = np.concatenate(rows)
    free = np.setdiff1d(np.arange(n), np.concatenate([rest[:, 0], rest[:, 1]]))
    assert len(free) >= 40, "the zoo needs untouched ids for its ruler path"
    ids = rng.permutation(free)[:32]
    ra, rb, rw = ruler_path(5)
    rows.append(np.stack([ids[ra], ids[rb], rw], axis=1))
    ops = np.concatenate(rows).astype(np.uint32)
    return ops[rng.permutation(len(ops))]


def ruler_path(k):
    """pairs and weights of the ruler path on 2^k vertices: edge {i - 1, i} has weight 1 + ctz(i); Boruvka hooks 2^(k-1), ...,
    2, 1 components in exactly k rounds.  Returns (a, b, w) int64 arrays"""
    i = np.arange(1, 1 << k, dtype=np.int64)
    ctz = np.zeros(len(i), np.int64)
    for bit in range(k):
        ctz[(i & ((1 << (bit + 1)) - 1)) == (1 << bit)] = bit
    return i - 1, i, 1 + ctz
