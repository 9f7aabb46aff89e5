"""numpy models of ppcsr_triangles / ppcsr_common_neighbours (include/ppcsr.h), built from the partitions' exported states.

Edge set: consumers_model.global_edges (live non-sentinel slots of every (beginning, end), slot N - 1 excluded, local src < n_p),
destinations >= n dropped.  Triangles use the upper orientation: {a, b}, a < b, is an edge exactly when the pair (a, b) is stored;
a triangle is a < b < c with (a, b), (a, c), (b, c) all stored.  model_triangles enumerates wedges — for every upper edge (a, b) the
upper neighbours c of b — and tests (a, c) by a sorted-key search; model_triangles_trace is an independent count for symmetric
graphs (trace(A^3) / 6 over dense uint64), which pins the convention."""
import numpy as np

from consumers_model import global_edges

WAVE_SLOTS = 4096  # kBfsWaveSlots: operand ranges beyond this many slots go to the deferred pass


def upper_edges(src, dst, n):
    """(a, b) of the stored pairs with a < b < n, ascending (a, b)"""
    ok = (dst < n) & (src < dst)
    a, b = src[ok].astype(np.int64), dst[ok].astype(np.int64)
    order = np.argsort(a * n + b, kind="stable")
    a, b = a[order], b[order]
    assert np.all(np.diff(a * n + b) > 0), "a (src, dst) pair is stored at most once"
    return a, b


def model_triangles(src, dst, n, chunk=1 << 22):
    """(tri uint64[n], total)"""
    a, b = upper_edges(src, dst, n)
    keys = a * n + b
    rows = np.searchsorted(a, np.arange(n + 1))
    deg = rows[1:] - rows[:-1]
    wedges = deg[b]  # per edge (a, b): the upper neighbours of b
    cum = np.concatenate([[0], np.cumsum(wedges)])
    tri = np.zeros(n, np.int64)
    total = 0
    e0 = 0
    while e0 < len(a):
        e1 = int(np.searchsorted(cum, cum[e0] + chunk, side="right")) - 1
        e1 = min(max(e1, e0 + 1), len(a))
        lens = wedges[e0:e1]
        tot = int(lens.sum())
        if tot:
            eidx = np.repeat(np.arange(e0, e1), lens)
            off = np.arange(tot) - np.repeat(cum[e0:e1] - cum[e0], lens)
            c = b[rows[b[eidx]] + off]
            q = a[eidx] * n + c
            pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
            hit = keys[pos] == q
            for v in (a[eidx][hit], b[eidx][hit], c[hit]):
                tri += np.bincount(v, minlength=n)
            total += int(hit.sum())
        e0 = e1
    assert int(tri.sum()) == 3 * total
    return tri.astype(np.uint64), total


def model_triangles_trace(src, dst, n):
    """triangles of a SYMMETRICALLY stored graph: trace(A^3) / 6 over dense uint64, self-loops dropped"""
    ok = (dst < n) & (src != dst)
    A = np.zeros((n, n), np.uint64)
    A[src[ok], dst[ok]] = 1
    assert np.array_equal(A, A.T), "the trace model needs both directions of every edge"
    t = int(np.einsum("ij,ji->", A @ A, A))
    assert t % 6 == 0
    return t // 6


def model_common_neighbours(src, dst, n, a, b):
    """counts[i] = stored destinations < n shared by a[i] and b[i] (np.intersect1d over CSR rows); vertices >= n give 0"""
    ok = dst < n
    s, d = src[ok].astype(np.int64), dst[ok].astype(np.int64)
    order = np.argsort(s * n + d, kind="stable")
    s, d = s[order], d[order]
    rows = np.searchsorted(s, np.arange(n + 1))
    out = np.zeros(len(a), np.uint32)
    for i, (x, y) in enumerate(zip(np.asarray(a).tolist(), np.asarray(b).tolist())):
        if x < n and y < n:
            out[i] = len(np.intersect1d(d[rows[x]:rows[x + 1]], d[rows[y]:rows[y + 1]], assume_unique=True))
    return out


def hardness(states, n, tri, total):
    """what keeps a parity test from passing on an easy input, from the model and the exported states alone"""
    src, dst = global_edges(states)
    h = dict(n=n, total=int(total), in_triangle=int(np.count_nonzero(tri)), backward=int(np.count_nonzero(src > dst)),
             loops=int(np.count_nonzero(src == dst)), beyond=int(np.count_nonzero(dst >= n)), gapped=0, long=0)
    rng_len = np.concatenate([nodes[:, 1].astype(np.int64) - nodes[:, 0].astype(np.int64) - 1 for _, _, nodes in states])
    for first, items, nodes in states:
        if not len(nodes):
            continue
        beg, end = nodes[:, 0].astype(np.int64), nodes[:, 1].astype(np.int64)
        nulls = np.concatenate([[0], np.cumsum(items[:, 2] == 0)])
        inside = nulls[np.maximum(end, beg + 1)] - nulls[beg + 1]
        h["gapped"] += int(np.count_nonzero((inside > 0) & (tri[first:first + len(nodes)] > 0)))
        # counted edges (a < b < n) whose operand — a's suffix behind the edge's slot, or b's range — is beyond one wave's reach
        live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)
        live[-1] = False
        live &= items[:, 0] < len(nodes)
        slot = np.nonzero(live)[0]
        a, b = items[slot, 0].astype(np.int64), items[slot, 1].astype(np.int64)
        counted = (a + first < b) & (b < n)
        slot, a, b = slot[counted], a[counted], b[counted]
        h["long"] += int(np.count_nonzero((end[a] - slot > WAVE_SLOTS) | (rng_len[b] > WAVE_SLOTS)))
    return h


def assert_hard(h, label="", want_long=False):
    n = h["n"]
    assert h["total"] >= n, (label, h)
    assert 16 * h["in_triangle"] >= n, (label, h)
    assert h["backward"] >= 1 and h["loops"] >= 1 and h["beyond"] >= 1, (label, h)
    assert h["gapped"] >= 1, (label, h)
    if want_long:
        assert h["long"] >= 1, (label, h)


# ---- which routine of pma_intersect.h answers what -------------------------------------------------------------------------------------
LANE_SLOTS, LOPSIDED = 32, 8  # kIsectLaneSlots, kIsectLopsided


def edge_counts(src, dst, n):
    """{(a, b): triangles (a, b, c), c > b} of the upper edges with a count above 0 (the wedge enumeration of model_triangles)"""
    a, b = upper_edges(src, dst, n)
    keys = a * n + b
    rows = np.searchsorted(a, np.arange(n + 1))
    lens = (rows[1:] - rows[:-1])[b]
    eidx = np.repeat(np.arange(len(a)), lens)
    off = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    c = b[rows[b[eidx]] + off]
    q = a[eidx] * n + c
    hit = keys[np.minimum(np.searchsorted(keys, q), len(keys) - 1)] == q
    cnt = np.bincount(eidx[hit], minlength=len(a))
    return {(int(x), int(y)): int(k) for x, y, k in zip(a[cnt > 0], b[cnt > 0], cnt[cnt > 0])}


def wave_route(la, lb):
    """the form of isect_wave for operands of la and lb slots"""
    s, l = min(la, lb), max(la, lb)
    return "wave_probe" if s and l // LOPSIDED > s else "wave_merge"


def routes(states, n):
    """Every counted edge (a, b) — a live non-sentinel slot s with a < b < n — classified by the slot lengths k_tri_edges and
    k_tri_long decide on: `aend - s` (one more than the slots of a's suffix behind the edge) and b's range (beginning, end) for
    lane / deferred; a's suffix and b's range from the first dest above b for the form of isect_wave.  From the exported states
    alone.  -> dict: route -> [edges, edges with a count above 0], and the counters of the glue code."""
    src, dst = global_edges(states)
    tri_of = edge_counts(src, dst, n)
    firsts = np.array([f for f, _, _ in states], np.int64)
    r = {k: [0, 0] for k in ("lane", "wave_merge", "wave_probe", "block")}
    c = dict(a_suffix={32: 0, 33: 0, WAVE_SLOTS: 0, WAVE_SLOTS + 1: 0}, mixed_chunks=0, full_quarter_chunks=0, credit_run_chunks=0, cross_partition=0,
             b_range_short=0, b_range_mid=0, b_range_long=0)
    for k, (first, items, nodes) in enumerate(states):
        if not len(nodes):
            continue
        live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)
        live[-1] = False
        live &= items[:, 0] < len(nodes)
        slot = np.nonzero(live)[0]
        la_, b_ = items[slot, 0].astype(np.int64), items[slot, 1].astype(np.int64)
        ok = (la_ + first < b_) & (b_ < n)
        slot, la_, b_ = slot[ok], la_[ok], b_[ok]
        aend = np.maximum(nodes[la_, 1].astype(np.int64), slot + 1)
        kb = np.searchsorted(firsts, b_, side="right") - 1
        lng = np.zeros(len(slot), bool)
        has = np.zeros(len(slot), bool)
        for i in range(len(slot)):
            s, a, b = int(slot[i]), int(la_[i]) + first, int(b_[i])
            _, bitems, bnodes = states[kb[i]]
            nb = bnodes[b - int(firsts[kb[i]])]
            bbeg = int(nb[0]) + 1
            bend = max(int(nb[1]), bbeg)
            suffix = int(aend[i]) - s
            if suffix in c["a_suffix"]:
                c["a_suffix"][suffix] += 1
            c["cross_partition"] += int(kb[i] != k)
            c["b_range_short" if bend - bbeg <= LANE_SLOTS else "b_range_mid" if bend - bbeg <= WAVE_SLOTS else "b_range_long"] += 1
            cnt = tri_of.get((a, b), 0)
            has[i] = cnt > 0
            if suffix > WAVE_SLOTS or bend - bbeg > WAVE_SLOTS:
                route, lng[i] = "block", True
            elif suffix <= LANE_SLOTS and bend - bbeg <= LANE_SLOTS:
                route = "lane"
            else:
                br = bitems[bbeg:bend]
                above = np.nonzero((br[:, 2] != 0) & (br[:, 1] > b))[0]
                blo = bbeg + int(above[0]) if len(above) else bend
                route = wave_route(suffix - 1, bend - blo)
            r[route][0] += 1
            r[route][1] += int(cnt > 0)
        chunk = slot // 64
        for ch in np.unique(chunk):
            m = chunk == ch
            if lng[m].any():
                c["mixed_chunks"] += int((~lng[m]).any())
                c["full_quarter_chunks"] += int(len(np.unique((slot[m][lng[m]] % 64) // 16)) == 4)
            c["credit_run_chunks"] += int(len(np.unique(la_[m][has[m]])) >= 3)
    return dict(routes=r, counters=c)


def assert_routes(rt, label="", partitions=1):
    """every route answers an edge that has triangles, and every seam of the glue code is met"""
    for name, (edges, with_tri) in rt["routes"].items():
        assert with_tri >= 1, (label, name, rt)
    c = rt["counters"]
    assert all(v >= 1 for v in c["a_suffix"].values()), (label, c)
    for key in ("mixed_chunks", "full_quarter_chunks", "credit_run_chunks", "b_range_short", "b_range_mid", "b_range_long"):
        assert c[key] >= 1, (label, key, c)
    if partitions > 1:  # (one partition has no such edge)
        assert c["cross_partition"] >= 1, (label, c)
