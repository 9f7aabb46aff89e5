"""numpy model of ppcsr_sample_neighbours / ppcsr_random_walks / ppcsr_degrees (include/ppcsr.h), restated from the definition and
built from the partitions' exported states [(first global vertex, items, nodes)] (consumers_model.partition_states).  Nothing
of the package is used: numpy and Python ints only.

  L(v)   the live slots of v's range (beginning, end) in slot order: non-null, non-sentinel, not slot N - 1, global dest < n
  W(v)   the sum of the measures of L(v): 1 each, or the edge values (weighted)
  draw   x = sm(sm(sm(seed) + i) + j), r = (x * W) >> 64, pick = the first entry whose inclusive cumulative measure exceeds r
"""
import numpy as np

from paths_model import global_edges_valued

NO_VERTEX = 0xFFFFFFFF
U = np.uint64
M32 = U(0xFFFFFFFF)


def sm(z):
    """splitmix64's finaliser on a uint64 array (arithmetic mod 2^64)"""
    with np.errstate(over="ignore"):
        z = np.asarray(z, U) + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def draw_x(seed, i, j):
    with np.errstate(over="ignore"):
        return sm(sm(sm(np.asarray([seed % (1 << 64)], U)) + np.asarray(i, U)) + np.asarray(j, U))


def mulhi(a, b):
    """high 64 bits of the 128-bit product, by 32-bit halves (no step overflows 64 bits)"""
    a, b = np.asarray(a, U), np.asarray(b, U)
    al, ah, bl, bh = a & M32, a >> U(32), b & M32, b >> U(32)
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> U(32)) + (lh & M32) + (hl & M32)
    return hh + (lh >> U(32)) + (hl >> U(32)) + (mid >> U(32))


def mulhi_int(a, b):
    return (int(a) * int(b)) >> 64


def neighbour_lists(states, n):
    """(rows int64[n + 1], dests uint32, values uint32): L(v) of every global vertex, read off the RANGES of the states"""
    cnt = np.zeros(n, np.int64)
    D, V, S = [np.empty(0, np.uint32)], [np.empty(0, np.uint32)], [np.empty(0, np.int64)]
    for first, items, nodes in states:
        m, N = len(nodes), len(items)
        if m == 0:
            continue
        lo = nodes[:, 0].astype(np.int64) + 1
        hi = nodes[:, 1].astype(np.int64)
        lens = np.maximum(hi - lo, 0)
        tot = int(lens.sum())
        idx = np.repeat(lo - np.cumsum(lens) + lens, lens) + np.arange(tot, dtype=np.int64)
        own = np.repeat(np.arange(m, dtype=np.int64), lens)
        it = items[idx]
        keep = (it[:, 2] != 0) & (it[:, 1] != 0xFFFFFFFF) & (it[:, 2] != 0xFFFFFFFF) & (idx != N - 1) & (it[:, 1].astype(np.int64) < n)
        D.append(it[keep, 1])
        V.append(it[keep, 2])
        S.append(own[keep] + first)
    src = np.concatenate(S)
    assert np.all(np.diff(src) >= 0), "vertex ranges out of order"
    cnt = np.bincount(src, minlength=n)
    rows = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return rows, np.concatenate(D).astype(np.uint32), np.concatenate(V).astype(np.uint32)


class Lists:
    def __init__(self, states, n, weighted):
        self.n = n
        self.rows, self.dests, self.values = neighbour_lists(states, n)
        meas = self.values.astype(U) if weighted else np.ones(len(self.dests), U)
        self.cum = np.concatenate([[0], np.cumsum(meas, dtype=U)]).astype(U)  # measure of the entries before entry e

    def pick(self, v, seed, i, j):
        """(dest, value) of draw (seed, i[q], j[q]) from L(v[q]) for arrays v, i, j; NO_VERTEX / 0 where there is nothing"""
        v = np.asarray(v, np.int64)
        ok = v < self.n
        vv = np.where(ok, v, 0)
        a, b = self.rows[vv], self.rows[vv + 1]
        ok &= b > a
        base = self.cum[a]
        W = np.where(ok, self.cum[b] - base, U(1)).astype(U)
        r = mulhi(draw_x(seed, i, j), W)
        e = np.searchsorted(self.cum, base + r, side="right").astype(np.int64) - 1
        e = np.where(ok, e, 0)
        assert np.all((e >= a) & (e < b) | ~ok)
        if len(self.dests) == 0:
            return np.full(len(v), NO_VERTEX, np.uint32), np.zeros(len(v), np.uint32)
        return (np.where(ok, self.dests[e], np.uint32(NO_VERTEX)).astype(np.uint32), np.where(ok, self.values[e], np.uint32(0)).astype(np.uint32))


def model_sample(states, n, vertices, fanout, seed=0, weighted=False):
    """(dests, values) uint32[k, fanout]"""
    q = np.asarray(vertices, np.uint32).reshape(-1)
    k = len(q)
    L = Lists(states, n, weighted)
    i = np.repeat(np.arange(k, dtype=U), fanout)
    j = np.tile(np.arange(fanout, dtype=U), k)
    d, val = L.pick(np.repeat(q.astype(np.int64), fanout), seed, i, j)
    return d.reshape(k, fanout), val.reshape(k, fanout)


def model_walks(states, n, starts, length, seed=0, weighted=False):
    """uint32[k, length + 1]"""
    q = np.asarray(starts, np.uint32).reshape(-1)
    k = len(q)
    L = Lists(states, n, weighted)
    out = np.empty((k, length + 1), np.uint32)
    out[:, 0] = np.where(q < n, q, np.uint32(NO_VERTEX))
    i = np.arange(k, dtype=U)
    for t in range(length):
        out[:, t + 1], _ = L.pick(out[:, t].astype(np.int64), seed, i, np.full(k, t, U))
    return out


def model_degrees(states, n):
    """(deg uint32[n], wsum uint64[n]) from the SOURCES of the live items (what one streaming pass sees): equal to |L(v)| and the
    weighted W(v) whenever every vertex's edges lie in its range"""
    src, dst, val = global_edges_valued(states)
    ok = dst < n
    deg = np.bincount(src[ok], minlength=n).astype(np.uint32)
    wsum = np.zeros(n, U)
    np.add.at(wsum, src[ok], val[ok].astype(U))
    return deg, wsum
