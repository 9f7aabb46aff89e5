"""CPU, no library: the two models of tests/community_model.py against each other on random graphs, against a brute force on every
small tie case, and against closed forms."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

from colouring_model import ORDER_DEGREE, ORDER_ID, ORDER_RANDOM
from community_model import (assert_maximisers, colours, decide, hardness, model_sweeps, modularity_ints, replica_sweeps, weighted_csr)


def rmat(streams, n, scale, m, seed):
    s, d = streams.rmat_edges_folded(n, scale, m, seed=seed)
    pairs = np.unique(np.stack([s, d], axis=1).astype(np.int64), axis=0)
    return pairs[:, 0], pairs[:, 1]


def both(src, dst, val, n, order, seed, weighted, init=None, max_sweeps=0):
    rows, nbr, wt = weighted_csr(src, dst, val, n, weighted)
    _, classes = colours(src, dst, n, order, seed)
    a = model_sweeps(rows, nbr, wt, classes, init, max_sweeps)
    b = replica_sweeps(rows, nbr, wt, classes, init, max_sweeps)
    np.testing.assert_array_equal(a["labels"], b["labels"])
    assert {k: v for k, v in a.items() if k != "labels"} == {k: v for k, v in b.items() if k != "labels"}
    if a["last"] == 0:
        assert_maximisers(rows, nbr, wt, a["labels"])
    return rows, nbr, wt, classes, a


@pytest.mark.parametrize("order", [ORDER_RANDOM, ORDER_DEGREE, ORDER_ID])
@pytest.mark.parametrize("weighted", [False, True])
def test_models_agree_on_random_graphs(streams, order, weighted):
    n = 700
    src, dst = rmat(streams, n, 10, 5000, seed=5)
    src = np.concatenate([src, [5, 3, 40]])  # a self-loop, a destination beyond n, a backward pair: no part of G
    dst = np.concatenate([dst, [5, n + 4, 2]])
    val = np.random.default_rng(order).integers(1, 4, len(src))  # (small weights: many ties)
    rows, nbr, wt, classes, r = both(src, dst, val, n, order, 9, weighted)
    h = hardness(rows, classes, r)
    assert h["sweeps"] >= 3 and h["classes"] >= 6 and h["own_ties"] >= 10 and h["min_ties"] >= 10 and h["wave_tier"] >= 1, h
    assert r["last"] == 0 and 1 < h["communities"] < n
    # stopping early, and a warm start from the converged answer: one sweep and no change
    for k in (1, 2):
        _, _, _, _, early = both(src, dst, val, n, order, 9, weighted, max_sweeps=k)
        assert early["sweeps"] == k and early["last"] > 0
    _, _, _, _, warm = both(src, dst, val, n, order, 9, weighted, init=r["labels"])
    assert warm["sweeps"] == 1 and warm["changes"] == 0
    np.testing.assert_array_equal(warm["labels"], r["labels"])


def brute_sweeps(n, edges, colour_order, init):
    """the definition once more, on dictionaries of the edge list itself"""
    label = list(init)
    sweeps = 0
    while True:
        sweeps += 1
        changed = 0
        for v in colour_order:
            scores = {}
            for a, b, w in edges:
                if v in (a, b):
                    other = a + b - v
                    scores[label[other]] = scores.get(label[other], 0) + w
            top = max(scores.values())
            if scores.get(label[v], 0) != top:
                label[v] = min(l for l, s in scores.items() if s == top)
                changed += 1
        if not changed:
            return label, sweeps


def test_models_against_brute_force_on_small_graphs():
    """every graph on 5 vertices that has an edge (all 1023 edge sets), with weights 1 and 2 on a fixed pattern, from the identity, a
    random and a crafted initial labelling, in the three orders and both flags"""
    n = 5
    pairs = list(itertools.combinations(range(n), 2))
    rng = np.random.default_rng(1)
    own = mins = 0
    for mask in range(1, 1 << len(pairs)):
        edges = [(a, b, 1 + (a + b) % 2) for i, (a, b) in enumerate(pairs) if mask >> i & 1]
        src, dst, val = (np.array(x, np.int64) for x in zip(*edges))
        for weighted in (False, True):
            rows, nbr, wt = weighted_csr(src, dst, val, n, weighted)
            for order in (ORDER_RANDOM, ORDER_DEGREE, ORDER_ID):
                colour, classes = colours(src, dst, n, order, mask)
                sequence = [int(v) for cl in classes for v in cl]
                for init in (None, rng.integers(0, n, n), np.array([4, 4, 0, 0, 2])):
                    a = model_sweeps(rows, nbr, wt, classes, init)
                    b = replica_sweeps(rows, nbr, wt, classes, init)
                    want, sweeps = brute_sweeps(n, [(x, y, w if weighted else 1) for x, y, w in edges], sequence,
                                                range(n) if init is None else init.tolist())
                    assert a["labels"].tolist() == want == b["labels"].tolist(), (mask, weighted, order, init)
                    assert a["sweeps"] == sweeps == b["sweeps"]
                    assert (a["own_ties"], a["min_ties"], a["changes"]) == (b["own_ties"], b["min_ties"], b["changes"])
                    own += a["own_ties"]
                    mins += a["min_ties"]
    assert own >= 10_000 and mins >= 10_000  # (both tie rules decided, many times)


def test_decide_tie_rules():
    assert decide({3: 5, 1: 5, 7: 2}, 3) == (3, True, False)   # the own label is one of several maxima: kept
    assert decide({3: 5, 1: 5, 7: 2}, 7) == (1, False, True)   # otherwise the smallest of them
    assert decide({3: 5, 1: 4}, 9) == (3, False, False)
    assert decide({2: (2 ** 32 - 2) * 3, 5: 2 ** 33}, 5) == (2, False, False)  # (sums beyond 32 bits compare as integers)


def test_closed_forms_and_modularity():
    """two disjoint cliques, identity start, id order: the first vertex takes the smallest label of its neighbours, the second
    keeps its own — one of several maxima — and everyone else follows; the modularity words by hand"""
    k = 6
    a = [(i, j) for i in range(k) for j in range(i + 1, k)]
    pairs = a + [(i + k, j + k) for i, j in a]
    src, dst = (np.array(x, np.int64) for x in zip(*pairs))
    val = np.ones(len(src), np.int64)
    n = 2 * k + 1  # (vertex 2 k is isolated)
    rows, nbr, wt, classes, r = both(src, dst, val, n, ORDER_ID, 0, False)
    assert r["labels"].tolist() == [1] * k + [k + 1] * k + [2 * k]
    words, s, q = modularity_ints(rows, nbr, wt, r["labels"])
    m = len(pairs)
    assert words == [2 * m, 2 * m, 2 * (m ** 2), 0] and s == 2 * m * m  # (each clique: tot = 2 * 15 = m)
    assert q == Fraction(1, 2)
    words, _, q = modularity_ints(rows, nbr, wt, np.zeros(n, np.int64))
    assert words == [2 * m, 2 * m, 4 * m * m, 0] and q == 0
    # weights near 2^32: the sum of squares needs the high word
    big = np.full(len(src), 2 ** 32 - 2, np.int64)
    rows, nbr, wt = weighted_csr(src, dst, big, n, True)
    words, s, q = modularity_ints(rows, nbr, wt, np.zeros(n, np.int64))
    assert words[3] > 0 and s == (2 * m * (2 ** 32 - 2)) ** 2 and q == 0
