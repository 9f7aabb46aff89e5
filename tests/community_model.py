"""Models of ppcsr_label_propagation / ppcsr_modularity (include/ppcsr.h), built from the partitions' exported states.  Nothing
of the package is used: numpy, and tests/colouring_model.py for the colours that schedule the sweeps.

G is the upper orientation (kcore_model.symmetric_csr's): {a, b}, a < b < n, is an edge exactly when the pair (a, b) is stored; its weight is the
stored value (weighted) or 1.
  weighted_csr      the symmetric CSR of G with the weight beside every entry
  colours           colour[] of the order and seed (colouring_model.levels), and the classes: the vertices of a colour that have
                    a neighbour
  model_sweeps      the definition: a sequential sweep in (colour, id) order on Python integers
  replica_sweeps    the steps as numpy: per class one sort of (vertex, label) and a run-length sum — a second route, and the
                    model where a Python loop would be too slow
  modularity_ints   the four words as Python ints and q as a Fraction
  hardness          what keeps a parity test from passing on an easy input; assert_hard (colouring_model) checks floors on it
  assert_maximisers a validator that does not know the order: after a converged call every vertex with a neighbour carries a
                    label of largest score"""
from fractions import Fraction

import numpy as np

from colouring_model import graph, levels

LANE_LIST, WAVE_LIST = 64, 512  # kLpLaneList, kLpWaveList: the longest lists of the first and the second tier
WEIGHTED = 1                    # PPCSR_COMMUNITY_WEIGHTED


def weighted_csr(src, dst, val, n, weighted):
    """(rows int64[n + 1], nbr int64[2 |E|], wt int64[2 |E|]): both directions of every upper edge, its weight beside it"""
    src, dst, val = np.asarray(src), np.asarray(dst), np.asarray(val)
    ok = (dst < n) & (src < dst)
    a, b, w = src[ok].astype(np.int64), dst[ok].astype(np.int64), val[ok].astype(np.int64)
    if not weighted:
        w = np.ones(len(a), np.int64)
    u, v, ww = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
    order = np.argsort(u, kind="stable")
    return np.searchsorted(u[order], np.arange(n + 1)), v[order], ww[order]


def colours(src, dst, n, order, seed):
    """(colour uint32[n], classes): classes[c] = the vertices of colour c with a neighbour, ascending — empty ones included"""
    rows, nbr, _, rank = graph(src, dst, n, order, seed)
    _, _, colour = levels(rows, nbr, rank)
    deg = rows[1:] - rows[:-1]
    ncol = int(colour.max()) + 1 if n else 0
    return colour, [np.nonzero((colour == c) & (deg > 0))[0] for c in range(ncol)]


def start_labels(n, init):
    return np.arange(n, dtype=np.int64) if init is None else np.asarray(init, np.int64).copy()


def decide(scores, own):
    """(label, own label among several maxima, the smallest of several maxima taken) for one vertex: scores = {label: weight}"""
    top = max(scores.values())
    best = [l for l, s in scores.items() if s == top]
    if scores.get(own, 0) == top:
        return own, len(best) > 1, False
    return min(best), False, len(best) > 1


def model_sweeps(rows, nbr, wt, classes, init=None, max_sweeps=0):
    """dict(labels, sweeps, changes, last, own_ties, min_ties): the sequential sweep, class after class, ids ascending"""
    n = len(rows) - 1
    label = start_labels(n, init).tolist()
    rows_l, nbr_l, wt_l = rows.tolist(), nbr.tolist(), wt.tolist()
    order = [v for cl in classes for v in cl.tolist()]
    sweeps = changes = last = own_ties = min_ties = 0
    while n:
        sweeps += 1
        last = 0
        for v in order:
            scores = {}
            for i in range(rows_l[v], rows_l[v + 1]):
                l = label[nbr_l[i]]
                scores[l] = scores.get(l, 0) + wt_l[i]
            now, t_own, t_min = decide(scores, label[v])
            own_ties += t_own
            min_ties += t_min
            if now != label[v]:
                label[v] = now
                last += 1
        changes += last
        if last == 0 or sweeps == max_sweeps:
            break
    return dict(labels=np.array(label, np.int64).astype(np.uint32), sweeps=sweeps, changes=changes, last=last, own_ties=own_ties,
                min_ties=min_ties)


def _expand(rows, front):
    lens = rows[front + 1] - rows[front]
    total = int(lens.sum())
    idx = np.repeat(rows[front] - np.cumsum(lens) + lens, lens) + np.arange(total)
    return np.repeat(np.arange(len(front)), lens), idx


def replica_step(rows, nbr, wt, label, cl):
    """one class, in place; (changes, own_ties, min_ties).  Sort the entries by (vertex, label), sum the runs, and per vertex
    take the first run of largest score — the smallest label — unless the own label's run reaches it"""
    who, idx = _expand(rows, cl)
    lab = label[nbr[idx]]
    order = np.lexsort((lab, who))
    who, lab, w = who[order], lab[order], wt[idx][order]
    head = np.ones(len(who), bool)
    head[1:] = (who[1:] != who[:-1]) | (lab[1:] != lab[:-1])
    at = np.nonzero(head)[0]
    rw, rl, rs = who[at], lab[at], np.add.reduceat(w, at)
    assert np.all(rs > 0)  # (int64 holds them: a weight is below 2^32 and a list below 2^31 entries)
    top = np.zeros(len(cl), np.int64)
    np.maximum.at(top, rw, rs)
    is_top = rs == top[rw]
    ntop = np.bincount(rw[is_top], minlength=len(cl))
    first_top = np.full(len(cl), len(rl), np.int64)
    np.minimum.at(first_top, rw[is_top], np.nonzero(is_top)[0])
    best = rl[first_top]
    own = label[cl]
    own_top = np.zeros(len(cl), bool)
    own_top[rw[is_top & (rl == own[rw])]] = True
    now = np.where(own_top, own, best)
    changed = now != own
    label[cl] = now
    return int(changed.sum()), int((own_top & (ntop > 1)).sum()), int((~own_top & (ntop > 1)).sum())


def replica_sweeps(rows, nbr, wt, classes, init=None, max_sweeps=0):
    """model_sweeps with numpy steps"""
    n = len(rows) - 1
    label = start_labels(n, init)
    sweeps = changes = last = own_ties = min_ties = 0
    while n:
        sweeps += 1
        last = 0
        for cl in classes:
            if len(cl):
                c, t_own, t_min = replica_step(rows, nbr, wt, label, cl)
                last += c
                own_ties += t_own
                min_ties += t_min
        changes += last
        if last == 0 or sweeps == max_sweeps:
            break
    return dict(labels=label.astype(np.uint32), sweeps=sweeps, changes=changes, last=last, own_ties=own_ties, min_ties=min_ties)


def _exact_sums(keys, w, size):
    """Python ints: per key the sum of the int64 weights w — two bincounts over 16-bit halves, each exact in float64 (a half sum
    stays below 2^53 for fewer than 2^37 entries)"""
    lo = np.bincount(keys, weights=(w & 0xFFFF).astype(np.float64), minlength=size)
    hi = np.bincount(keys, weights=(w >> 16).astype(np.float64), minlength=size)
    return [int(a) + (int(b) << 16) for a, b in zip(lo.tolist(), hi.tolist())]


def modularity_ints(rows, nbr, wt, labels):
    """(words [2 W, 2 in, S low, S high], S, q as a Fraction) on Python ints"""
    n = len(rows) - 1
    labels = np.asarray(labels, np.int64)
    owner = np.repeat(np.arange(n), rows[1:] - rows[:-1])
    inside = (labels[owner] == labels[nbr]).astype(np.int64)
    two_w, two_in = (_exact_sums(np.zeros(len(wt), np.int64), x, 1)[0] for x in (wt, wt * inside))
    tot = _exact_sums(labels[owner], wt, n) if n else []
    s = sum(t * t for t in tot)
    q = Fraction(two_in, two_w) - Fraction(s, two_w * two_w) if two_w else Fraction(0)
    return [two_w, two_in, s & (2 ** 64 - 1), s >> 64], s, q


def hardness(rows, classes, result):
    deg = rows[1:] - rows[:-1]
    return dict(n=len(deg), edges=int(rows[-1]) // 2, sweeps=result["sweeps"], classes=sum(1 for cl in classes if len(cl)),
                changes=result["changes"], communities=len(np.unique(result["labels"])), own_ties=result["own_ties"],
                min_ties=result["min_ties"], lane_tier=int(np.count_nonzero((deg > 0) & (deg <= LANE_LIST))),
                wave_tier=int(np.count_nonzero((deg > LANE_LIST) & (deg <= WAVE_LIST))), block_tier=int(np.count_nonzero(deg > WAVE_LIST)),
                widest_class=max((len(cl) for cl in classes), default=0),
                class0_lane_tier=int(np.count_nonzero(deg[classes[0]] <= LANE_LIST)) if classes else 0, maxdeg=int(deg.max()) if len(deg) else 0,
                isolated=int(np.count_nonzero(deg == 0)))


def assert_maximisers(rows, nbr, wt, labels, label=""):
    """every vertex with a neighbour carries a label of largest score among its neighbours' labels"""
    n = len(rows) - 1
    labels = np.asarray(labels, np.int64)
    front = np.nonzero(rows[1:] > rows[:-1])[0]
    who, idx = _expand(rows, front)
    lab = labels[nbr[idx]]
    order = np.lexsort((lab, who))
    who, lab, w = who[order], lab[order], wt[idx][order]
    head = np.ones(len(who), bool)
    head[1:] = (who[1:] != who[:-1]) | (lab[1:] != lab[:-1])
    at = np.nonzero(head)[0]
    rw, rl, rs = who[at], lab[at], (np.add.reduceat(w, at) if len(at) else np.empty(0, np.int64))
    top = np.zeros(len(front), np.int64)
    np.maximum.at(top, rw, rs)
    own = np.zeros(len(front), np.int64)
    mine = rl == labels[front][rw]
    own[rw[mine]] = rs[mine]
    assert np.all(own == top), (label, "a vertex carries a label that is not a maximiser", front[own != top][:5])
