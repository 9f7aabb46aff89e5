"""Host model of ppcsr_scc / pppcsr_scc (include/ppcsr.h): strongly connected components of the directed graph whose edges are
consumers_model.global_edges(partition_states(pp)) — destinations >= n skipped, values ignored — every SCC named by its smallest
vertex id.  An iterative Tarjan on Python integers; beside it the set the exhaustive trim of the whole graph retires, the
conditions an input must meet before a parity test on it counts (hardness / assert_hard, as paths_model and kcore_model), the
zoo — the generator of the graphs both test files use — and a synchronous numpy replica of the device schedule, whose pass
counts tools/scc_bench.py puts beside the device's.  Nothing here imports the package."""
import numpy as np


def _csr(src, dst, n):
    """(rows, d) of the edges with dst < n, grouped by source"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ok = dst < n
    s, d = src[ok], dst[ok]
    order = np.argsort(s, kind="stable")
    s, d = s[order], d[order]
    return np.searchsorted(s, np.arange(n + 1)), d


def model_scc(src, dst, n):
    """labels (uint32[n]): the smallest vertex id of every vertex's SCC.  Tarjan's algorithm with an explicit call stack."""
    rows, d = _csr(src, dst, n)
    rows, d = rows.tolist(), d.tolist()
    index = [-1] * n
    low = [0] * n
    on = [False] * n
    labels = [0] * n
    stack = []
    nxt = 0
    for root in range(n):
        if index[root] != -1:
            continue
        index[root] = low[root] = nxt
        nxt += 1
        stack.append(root)
        on[root] = True
        call = [(root, rows[root])]
        while call:
            v, i = call[-1]
            if i < rows[v + 1]:
                call[-1] = (v, i + 1)
                w = d[i]
                if index[w] == -1:
                    index[w] = low[w] = nxt
                    nxt += 1
                    stack.append(w)
                    on[w] = True
                    call.append((w, rows[w]))
                elif on[w] and index[w] < low[v]:
                    low[v] = index[w]
                continue
            call.pop()
            if call:
                u = call[-1][0]
                if low[v] < low[u]:
                    low[u] = low[v]
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                m = min(comp)
                for w in comp:
                    labels[w] = m
    return np.array(labels, np.uint32) if n else np.empty(0, np.uint32)


def trim_closure(src, dst, n):
    """(retired, sweeps): the vertices the exhaustive trim of the WHOLE graph retires (bool[n]) — a vertex goes when it has no
    in-neighbour or no out-neighbour other than itself among those left — and the number of synchronous sweeps that retired
    something.  The set is unique (trimming is monotone: what may go stays removable when more has gone); the sweep count is
    that of the synchronous schedule."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ok = (dst < n) & (src != dst)
    s, d = src[ok], dst[ok]
    live = np.ones(n, bool)
    sweeps = 0
    while True:
        e = live[s] & live[d]
        has_out, has_in = np.zeros(n, bool), np.zeros(n, bool)
        has_out[s[e]] = True
        has_in[d[e]] = True
        go = live & ~(has_out & has_in)
        if not go.any():
            return ~live, sweeps
        live &= ~go
        sweeps += 1


def _reach(rows, d, n, starts):
    seen = np.zeros(n, bool)
    seen[starts] = True
    front = np.asarray(starts, np.int64)
    while len(front):
        a, lens = rows[front], rows[front + 1] - rows[front]
        idx = np.repeat(a - np.cumsum(lens) + lens, lens) + np.arange(int(lens.sum()))
        nb = np.unique(d[idx])
        front = nb[~seen[nb]]
        seen[front] = True
    return seen


def hardness(src, dst, n, labels):
    """what an input exercises, from the model's labels"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    sizes = np.bincount(labels.astype(np.int64), minlength=n) if n else np.zeros(0, np.int64)
    nontrivial = np.flatnonzero(sizes > 1)
    h = dict(nontrivial=len(nontrivial), distinct=len(np.unique(sizes[nontrivial])), largest=int(sizes.max()) if n else 0,
             trim_sweeps=trim_closure(src, dst, n)[1], below=0, above=0, beyond=int((dst >= n).sum()))
    ok = dst < n
    loop = np.zeros(n, bool)
    loop[src[ok & (src == dst)]] = True
    h["loops"] = int((loop & (sizes[labels.astype(np.int64)] == 1)).sum()) if n else 0
    h["max_out"] = int(np.bincount(src[ok], minlength=n).max()) if ok.any() else 0
    h["max_in"] = int(np.bincount(dst[ok], minlength=n).max()) if ok.any() else 0
    if len(nontrivial):
        big = int(np.argmax(sizes))  # (the label of the largest SCC is one of its vertices)
        rows, d = _csr(src, dst, n)
        rows_t, d_t = _csr(dst[ok], src[ok], n)
        other = (sizes[labels.astype(np.int64)] > 1) & (labels != big)
        h["below"] = len(np.unique(labels[_reach(rows, d, n, [big]) & other]))      # non-trivial SCCs the largest reaches
        h["above"] = len(np.unique(labels[_reach(rows_t, d_t, n, [big]) & other]))  # non-trivial SCCs that reach it
    return h


def assert_hard(h, label, **floors):
    """every key of floors is a lower bound on h[key]"""
    for key, least in floors.items():
        assert h[key] >= least, f"{label}: the input is too easy: {key} = {h[key]} < {least} ({h})"


def geometric_lengths(count, longest):
    """`count` distinct cycle lengths from 2 to `longest`, geometrically spaced"""
    out = sorted({int(round(2 * (longest / 2) ** (i / (count - 1)))) for i in range(count)})
    return out


def zoo(streams, n, scale, core_edges, cycles, longest, k, L, seed):
    """Rows (src, dst, 1) of a graph with many SCC shapes — a plain RMAT graph has ONE non-trivial SCC and never enters the
    colouring phase.  A folded RMAT core; a sorted pool of ids from the upper three quarters, whose core edges are dropped;
    planted on the pool, ids ascending in pool order unless said otherwise: `cycles` directed cycles of geometrically spaced
    lengths up to `longest`, each in a permuted vertex order; a chain of k two-cycles a_i <-> b_i, b_i -> a_(i+1), with ids
    ascending along the chain (k colouring rounds) and one with ids descending (one round); a cycle of L vertices in ascending
    id order; two paths of L single vertices, ascending and descending, the first with a self-loop on every 7th vertex; a cycle
    with an edge INTO the core's largest-out-degree vertex and one with an edge FROM it; four isolated vertices with
    self-loops and a dozen without; a few rows with dst >= n."""
    rng = np.random.default_rng(seed)
    lengths = geometric_lengths(cycles, longest)
    need = sum(lengths) + 4 * k + 3 * L + 5 + 6 + 4 + 12
    assert need <= n - n // 4, (need, n)
    pool = np.sort(rng.choice(np.arange(n // 4, n), need, replace=False)).astype(np.int64)
    s, d = streams.rmat_edges_folded(n, scale, core_edges, seed=seed)
    s, d = s.astype(np.int64), d.astype(np.int64)
    in_pool = np.zeros(n, bool)
    in_pool[pool] = True
    keep = ~(in_pool[s] | in_pool[d])
    s, d = s[keep], d[keep]
    hub = int(np.argmax(np.bincount(s[s != d], minlength=n)))
    pos = 0

    def take(m):
        nonlocal pos
        pos += m
        return pool[pos - m:pos]

    pairs = []

    def ring(ids):
        pairs.append(np.stack([ids, np.roll(ids, -1)], axis=1))

    for m in lengths:
        ring(rng.permutation(take(m)))
    for ids in (take(2 * k), take(2 * k)[::-1]):  # the chain: ascending, then descending along the edges
        a, b = ids[0::2], ids[1::2]
        pairs += [np.stack([a, b], axis=1), np.stack([b, a], axis=1), np.stack([b[:-1], a[1:]], axis=1)]
    ring(take(L))
    up, down = take(L), take(L)[::-1]
    pairs += [np.stack([up[:-1], up[1:]], axis=1), np.stack([down[:-1], down[1:]], axis=1), np.stack([up[::7], up[::7]], axis=1)]
    into, out_of = take(5), take(6)
    ring(into)
    ring(out_of)
    pairs += [np.array([[into[2], hub], [hub, out_of[3]]], np.int64)]
    loops = take(4)
    pairs.append(np.stack([loops, loops], axis=1))
    take(12)  # isolated
    assert pos == need
    far = np.stack([s[:5], np.full(5, n, np.int64) + np.arange(5)], axis=1)  # destinations >= n
    rows = np.concatenate([np.stack([s, d], axis=1)] + pairs + [far])
    rows = rows[rng.permutation(len(rows))]
    return np.concatenate([rows, np.ones((len(rows), 1), np.int64)], axis=1).astype(np.uint32)


def replica(src, dst, n, pivot=None):
    """(labels, counts): a SYNCHRONOUS numpy replica of the device schedule — trim to a fixpoint, forward-backward reach from
    one pivot (the live vertex of the largest out-degree, ties to the smaller id, unless given), colouring rounds, the trim
    after each — in which every pass reads the state the pass before it left.  counts: the passes of every loop, each
    including the last pass, which finds nothing; the device reads marks as they are, so it should need no more."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ok = (dst < n) & (src != dst)
    s, d = src[ok], dst[ok]
    scc = np.full(n, -1, np.int64)
    c = dict(trim_sweeps=0, trimmed=0, fw_passes=0, bw_passes=0, pivot=None, pivot_scc=0, rounds=0, prop_passes=0, reach_passes=0, coloured=0)

    def trim():
        while (scc < 0).any():
            live = scc < 0
            e = live[s] & live[d]
            has_out, has_in = np.zeros(n, bool), np.zeros(n, bool)
            has_out[s[e]] = True
            has_in[d[e]] = True
            go = live & ~(has_out & has_in)
            scc[go] = np.flatnonzero(go)
            c["trim_sweeps"] += 1
            c["trimmed"] += int(go.sum())
            if not go.any():
                break

    def reach(seed, a, b, key, same=None):
        """marks travel along a -> b inside the live graph, one hop per pass"""
        mark = seed.copy()
        live = scc < 0
        while True:
            c[key] += 1
            e = mark[a] & live[b] & ~mark[b]
            if same is not None:
                e &= same[a] == same[b]
            if not e.any():
                return mark
            mark[b[e]] = True

    trim()
    if (scc < 0).any():
        live = scc < 0
        if pivot is None:
            deg = np.bincount(s[live[s] & live[d]], minlength=n)
            deg[~live] = -1
            pivot = int(np.argmax(deg))
        assert live[pivot]
        seed = np.zeros(n, bool)
        seed[pivot] = True
        both = reach(seed, s, d, "fw_passes") & reach(seed, d, s, "bw_passes")
        scc[both] = np.flatnonzero(both).min()
        c["pivot"], c["pivot_scc"] = int(pivot), int(both.sum())
        trim()
    while (scc < 0).any():
        c["rounds"] += 1
        live = scc < 0
        colour = np.where(live, np.arange(n), n)
        e = live[s] & live[d]
        a, b = s[e], d[e]
        while True:
            c["prop_passes"] += 1
            new = colour.copy()
            np.minimum.at(new, b, colour[a])
            if np.array_equal(new, colour):
                break
            colour = new
        marked = reach(live & (colour == np.arange(n)), d, s, "reach_passes", same=colour)
        scc[marked] = colour[marked]
        c["coloured"] += int(marked.sum())
        trim()
    return scc.astype(np.uint32), c
