"""The hand-built graph of the sampling tests (n = 2^12), as a list of adds plus a few deletes: one vertex per case the kernels of
pma_sample.h tell apart.  A bulk build places element number e of the sequence (sentinel 0, edges of 0, sentinel 1, ...) at
po_redistribute_positions(0, N, j)[e], whoever owns it (tests/bulk_model.py), so with the number of edges held fixed the slot
range of a vertex is a function of its first element and its degree alone: the two vertices at the per-wave threshold get
their degrees — and the vertices in front of them their padding — from a search of that position table."""
import numpy as np

from bulk_model import array_size
from oracle_lib import oracle_lib

N_VERT = 1 << 12
WAVE_SLOTS = 4096      # kBfsWaveSlots
HUB_EDGES = 300000
TOTAL_EDGES = 340000   # held fixed: the slack vertex takes what the others leave
BIG = (1 << 32) - 2    # the largest value an edge can carry

# vertex ids, ascending in the order the array holds them
V = dict(deg0=0, deg1=1, deg63=2, deg64=3, deg65=4, deg127=5, beyond=6, loop=7, pad_a=50, exact=51, pad_b=60, over=61, hub=70, slack=80,
         gone=4090)


def _edges(v, dests, rng, heavy=False):
    dests = np.asarray(dests, np.uint32)
    vals = rng.integers(1, 1 << 16, len(dests)).astype(np.uint32)
    if heavy and len(dests):
        vals[rng.random(len(dests)) < 0.5] = 1
        vals[:: 3] = BIG - (np.arange(len(vals[:: 3]), dtype=np.uint32) % np.uint32(5))
    return np.stack([np.full(len(dests), v, np.uint32), dests, vals], 1)


def hand_graph(N0, seed=1):
    """-> (adds, deletes, want): adds for a bulk build (or a batch) into an array of N0 slots, deletes to apply afterwards,
    want[name] = (vertex, range length in slots or None) for the vertices whose range the build pins"""
    n = N_VERT
    rng = np.random.default_rng(seed)
    E = TOTAL_EDGES
    j = n + E
    N = array_size(n, N0, E)
    pos = np.zeros(j, np.uint64)
    oracle_lib().po_redistribute_positions(0, N, j, pos.ctypes.data)
    pos = pos.astype(np.int64)
    deg = {V["deg1"]: 1, V["deg63"]: 63, V["deg64"]: 64, V["deg65"]: 65, V["deg127"]: 127, V["beyond"]: 40, V["loop"]: 1, V["gone"]: 30}

    def fit(vertex, pad, slots):
        """degree of `vertex` and of its padding vertex such that (beginning, end) of `vertex` holds exactly `slots` slots"""
        before = sum(d for u, d in deg.items() if u < pad)
        a = vertex + before + np.arange(0, 3000)  # the vertex's sentinel element, for every padding degree
        k = np.searchsorted(pos, pos[a] + slots + 1)
        hit = np.nonzero((k < j) & (pos[np.minimum(k, j - 1)] == pos[a] + slots + 1))[0]
        assert len(hit), "no degree gives this range length"
        deg[pad] = int(hit[0])
        deg[vertex] = int(k[hit[0]] - a[hit[0]] - 1)

    fit(V["exact"], V["pad_a"], WAVE_SLOTS)
    fit(V["over"], V["pad_b"], WAVE_SLOTS + 1)
    deg[V["hub"]] = HUB_EDGES
    deg[V["slack"]] = E - sum(deg.values())
    assert deg[V["slack"]] > 0
    parts = []
    for u, d in sorted(deg.items()):
        if u == V["beyond"]:
            dests = n + rng.permutation(5000)[:d]
        elif u == V["loop"]:
            dests = [u]
        elif u in (V["hub"], V["slack"]):
            dests = rng.permutation(max(d, n) + 1000)[:d]  # (most of a hub's dests lie beyond n: chunks of measure 0)
            dests[: 8] = [u, 0, 1, 2, n - 1, V["hub"], V["exact"], V["over"]]
            dests = np.unique(dests)
            extra = np.setdiff1d(np.arange(d + 5000), dests)[: d - len(dests)]
            dests = np.concatenate([dests, extra])
        else:
            dests = rng.permutation(n)[:d]  # every one a vertex
            if d > 200:
                dests[: d // 7] += n  # with some beyond the graph among them
                dests = np.unique(dests)
                dests = np.concatenate([dests, np.setdiff1d(np.arange(n), dests)[: d - len(dests)]])
        assert len(np.unique(dests)) == d == len(dests), (u, d)
        parts.append(_edges(u, dests, rng, heavy=u in (V["hub"], V["exact"], V["deg65"], V["deg127"])))
    adds = np.concatenate(parts).astype(np.uint32)
    adds = adds[rng.permutation(len(adds))]
    assert len(adds) == E
    gone = adds[adds[:, 0] == V["gone"]]
    deletes = np.stack([gone[:, 0], gone[:, 1], np.zeros(len(gone), np.uint32)], 1)
    want = {"exact": (V["exact"], WAVE_SLOTS), "over": (V["over"], WAVE_SLOTS + 1), "hub": (V["hub"], None)}
    return adds, deletes, want


def hand_queries(rng, k):
    """k query vertices: the named vertices, their neighbours in id, vertices >= n; the rest drawn so that half start on the hub"""
    n = N_VERT
    named = np.array(sorted(set(V.values())) + [n, n + 3, 0xFFFFFFFF, V["hub"], V["hub"], V["exact"]], np.uint32)
    rest = k - len(named)
    fill = np.where(rng.random(rest) < 0.5, V["hub"], rng.integers(0, n + 4, rest)).astype(np.uint32)
    q = np.concatenate([named, fill])
    return q[rng.permutation(len(q))]
