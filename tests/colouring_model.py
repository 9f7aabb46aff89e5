"""Models of ppcsr_colouring / ppcsr_mis (include/ppcsr.h), built from the partitions' exported states.  Nothing of the package
is used: numpy, sampling_model.draw_x for the keys and kcore_model.symmetric_csr for the graph.

G is the upper orientation (kcore_model): {a, b}, a < b < n, is an edge exactly when the pair (a, b) is stored.
Order: u precedes w iff key[u] > key[w], or the keys are equal and u < w (model_keys, order_of).
  model_colouring   sequential greedy colouring in that order, on Python ints: the definition
  model_mis         the lexicographically first MIS in that order, likewise
  levels            the levels of the order's DAG by a synchronous numpy peel — rounds and frontier sizes of the colouring — and,
                    level by level, the greedy colours again: an independent second route to model_colouring
  mis_rounds        a synchronous numpy replica of the MIS rounds over the edge list: the round counters, and a second route
                    to model_mis (also the model where a Python loop would be too slow)
  hardness          what keeps a parity test from passing on an easy input; assert_hard checks floors on it
  assert_proper, assert_maximal_independent     validators that do not know the order"""
import numpy as np

from kcore_model import symmetric_csr
from sampling_model import draw_x
from triangles_model import upper_edges

ORDER_RANDOM, ORDER_DEGREE, ORDER_ID = 0, 1, 2
WAVE_SLOTS = 4096  # kBfsWaveSlots: a longer list is left to the long-list kernel
U = np.uint64


def model_keys(order, seed, n, degree):
    """key uint64[n] of the table in include/ppcsr.h; degree = deg_G"""
    if order == ORDER_ID:
        return np.zeros(n, U)
    draw = draw_x(seed, np.arange(n, dtype=U), 0)
    if order == ORDER_RANDOM:
        return draw
    assert order == ORDER_DEGREE
    return (np.asarray(degree, U) << U(32)) | (draw >> U(32))


def order_of(keys):
    """the vertices in the order: descending key, ties by ascending id"""
    return np.lexsort((np.arange(len(keys)), ~np.asarray(keys, U)))


def graph(src, dst, n, order, seed):
    """(rows, nbr, keys, rank): the symmetric CSR of G, the keys and rank[v] = v's place in the order"""
    rows, nbr = symmetric_csr(src, dst, n)
    keys = model_keys(order, seed, n, rows[1:] - rows[:-1])
    rank = np.empty(n, np.int64)
    rank[order_of(keys)] = np.arange(n)
    return rows, nbr, keys, rank


def model_colouring(rows, nbr, keys):
    """colour uint32[n]: the vertices in the order, each the smallest colour none of its coloured neighbours carries"""
    n = len(rows) - 1
    colour = [-1] * n
    rows_l, nbr_l = rows.tolist(), nbr.tolist()
    for v in order_of(keys).tolist():
        taken = {colour[w] for w in nbr_l[rows_l[v]:rows_l[v + 1]]}
        c = 0
        while c in taken:
            c += 1
        colour[v] = c
    return np.array(colour, np.int64).astype(np.uint32)


def model_mis(rows, nbr, keys):
    """mask bool[n]: the vertices in the order, each a member unless a neighbour already is"""
    n = len(rows) - 1
    member = [False] * n
    rows_l, nbr_l = rows.tolist(), nbr.tolist()
    for v in order_of(keys).tolist():
        member[v] = not any(member[w] for w in nbr_l[rows_l[v]:rows_l[v + 1]])
    return np.array(member, bool)


def _expand(rows, front):
    """(owner index into front, neighbour) of every list entry of the vertices in front"""
    lens = rows[front + 1] - rows[front]
    total = int(lens.sum())
    idx = np.repeat(rows[front] - np.cumsum(lens) + lens, lens) + np.arange(total)
    return np.repeat(np.arange(len(front)), lens), idx


def levels(rows, nbr, rank):
    """(level int64[n], sizes list, colour uint32[n]): level 0 = no preceding neighbour, else 1 + the largest level of one;
    sizes[r] = vertices at level r; the colours computed level by level (a level's vertices are pairwise non-adjacent and all
    their preceding neighbours lie in earlier levels)"""
    n = len(rows) - 1
    owner = np.repeat(np.arange(n), rows[1:] - rows[:-1])
    pred = np.bincount(owner[rank[nbr] < rank[owner]], minlength=n)
    level = np.full(n, -1, np.int64)
    colour = np.full(n, -1, np.int64)
    sizes = []
    front = np.nonzero(pred == 0)[0]
    while len(front):
        r = len(sizes)
        sizes.append(len(front))
        who, idx = _expand(rows, front)
        w = nbr[idx]
        done = colour[w] >= 0
        # mex per frontier vertex: its distinct neighbour colours ascending — the first place where colour != position
        pairs = np.unique(who[done] * (n + 1) + colour[w[done]])
        pv, pc = pairs // (n + 1), pairs % (n + 1)
        start = np.searchsorted(pv, np.arange(len(front)))
        count = np.searchsorted(pv, np.arange(len(front)), side="right") - start
        pos = np.arange(len(pairs)) - start[pv]
        miss = np.full(len(front), n + 1, np.int64)
        np.minimum.at(miss, pv[pc != pos], pos[pc != pos])
        level[front] = r
        colour[front] = np.where(miss <= n, miss, count)
        nxt = w[~done]
        pred -= np.bincount(nxt, minlength=n)
        cand = np.unique(nxt)
        front = cand[pred[cand] == 0]
    assert not n or level.min() >= 0, "the order's DAG left vertices without a level"
    return level, sizes, colour.astype(np.uint32)


UNDECIDED, IN, OUT = 2, 1, 0


def mis_rounds(src, dst, n, rank):
    """(mask bool[n], dict(rounds, members1, undecided1, size)): round r — against the state of round r - 1, an IN end of an
    edge marks the other end out and, if both ends are undecided, the succeeding end is blocked; then every undecided vertex
    marked out goes OUT and every one neither marked nor blocked goes IN"""
    a, b = upper_edges(np.asarray(src), np.asarray(dst), n)
    first = np.where(rank[a] < rank[b], a, b)
    second = a + b - first
    state = np.full(n, UNDECIDED, np.int8)
    rounds = members1 = undecided1 = 0
    left = n
    while left:
        rounds += 1
        assert rounds <= 2 * n + 1
        sa, sb = state[a], state[b]
        out = np.zeros(n, bool)
        out[b[(sa == IN) & (sb == UNDECIDED)]] = True
        out[a[(sb == IN) & (sa == UNDECIDED)]] = True
        blocked = np.zeros(n, bool)
        blocked[second[(sa == UNDECIDED) & (sb == UNDECIDED)]] = True
        und = state == UNDECIDED
        state[und & out] = OUT
        state[und & ~out & ~blocked] = IN
        left = int(np.count_nonzero(state == UNDECIDED))
        if rounds == 1:
            members1, undecided1 = int(np.count_nonzero(state == IN)), left
        # (edges with a decided end that has done its marking no longer matter)
        keep = (state[a] != OUT) & (state[b] != OUT)
        a, b, first, second = a[keep], b[keep], first[keep], second[keep]
    mask = state == IN
    return mask, dict(rounds=rounds, members1=members1, undecided1=undecided1, size=int(np.count_nonzero(mask)))


def hardness(src, dst, n, rows, colour, sizes):
    src, dst = np.asarray(src), np.asarray(dst)
    degree = rows[1:] - rows[:-1]
    return dict(n=n, edges=int(rows[-1]) // 2, ncolours=int(colour.max()) + 1 if n else 0, rounds=len(sizes), widest=max(sizes) if sizes else 0,
                maxdeg=int(degree.max()) if n else 0, long_lists=int(np.count_nonzero(degree > WAVE_SLOTS)),
                isolated=int(np.count_nonzero(degree == 0)), backward=int(np.count_nonzero(src > dst)),
                loops=int(np.count_nonzero(src == dst)), beyond=int(np.count_nonzero(dst >= n)))


def assert_hard(h, label="", **at_least):
    """every named field of hardness() is at least the given value"""
    for key, bound in at_least.items():
        assert h[key] >= bound, (label, key, bound, h)


def assert_proper(rows, nbr, colour, label=""):
    """no edge of G joins equal colours, and every colour c > 0 of v has all of 0 .. c - 1 among v's neighbours (a greedy
    colouring in SOME order) — hence colour[v] <= deg(v)"""
    n = len(rows) - 1
    colour = np.asarray(colour).astype(np.int64)
    owner = np.repeat(np.arange(n), rows[1:] - rows[:-1])
    cn = colour[nbr]
    assert not np.any(cn == colour[owner]), (label, "an edge joins two vertices of one colour")
    below = cn < colour[owner]
    distinct = np.unique(owner[below] * (n + 1) + cn[below]) // (n + 1)
    np.testing.assert_array_equal(np.bincount(distinct, minlength=n), colour, err_msg=f"{label}: a smaller colour was free")
    assert np.all(colour <= rows[1:] - rows[:-1]), label


def assert_maximal_independent(rows, nbr, mask, label=""):
    n = len(rows) - 1
    mask = np.asarray(mask).astype(bool)
    owner = np.repeat(np.arange(n), rows[1:] - rows[:-1])
    assert not np.any(mask[owner] & mask[nbr]), (label, "two members are adjacent")
    covered = np.bincount(owner[mask[nbr]], minlength=n) > 0
    assert np.all(mask | covered), (label, "a vertex outside the set has no member among its neighbours")
