"""CPU, no library: the models of tests/colouring_model.py against networkx and against closed forms."""
import numpy as np
import pytest

from colouring_model import (ORDER_DEGREE, ORDER_ID, ORDER_RANDOM, assert_maximal_independent, assert_proper, graph, levels, mis_rounds,
                             model_colouring, model_keys, model_mis, order_of)
from sampling_model import draw_x


def rmat(streams, n, scale, m, seed):
    s, d = streams.rmat_edges_folded(n, scale, m, seed=seed)
    pairs = np.unique(np.stack([s, d], axis=1).astype(np.int64), axis=0)
    return pairs[:, 0], pairs[:, 1]


def both_routes(src, dst, n, order, seed):
    """the four models on one input; the two routes to each result agree and the validators pass"""
    rows, nbr, keys, rank = graph(src, dst, n, order, seed)
    colour = model_colouring(rows, nbr, keys)
    level, sizes, colour2 = levels(rows, nbr, rank)
    np.testing.assert_array_equal(colour, colour2)
    mask = model_mis(rows, nbr, keys)
    mask2, rounds = mis_rounds(src, dst, n, rank)
    np.testing.assert_array_equal(mask, mask2)
    np.testing.assert_array_equal(mask, colour == 0)
    assert rounds["size"] == np.count_nonzero(mask) and rounds["members1"] == (sizes[0] if n else 0)  # (the local maxima are level 0)
    assert_proper(rows, nbr, colour)
    assert_maximal_independent(rows, nbr, mask)
    assert sum(sizes) == n and rounds["rounds"] <= 2 * len(sizes)
    return rows, nbr, keys, colour, mask, sizes, rounds


@pytest.mark.parametrize("order", [ORDER_RANDOM, ORDER_DEGREE, ORDER_ID])
def test_model_against_networkx(streams, order):
    """networkx.greedy_color with a strategy that returns the model's order: the same colours; its colour 0 is the model's MIS"""
    nx = pytest.importorskip("networkx")
    n = 900
    src, dst = rmat(streams, n, 10, 7000, seed=17)
    src = np.concatenate([src, [5, 3, 40]])  # a self-loop, a destination beyond n, a backward pair: no part of G
    dst = np.concatenate([dst, [5, n + 4, 2]])
    rows, nbr, keys, colour, mask, sizes, _ = both_routes(src, dst, n, order, seed=11)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from((v, int(w)) for v in range(n) for w in nbr[rows[v]:rows[v + 1]] if v < w)
    ref = nx.greedy_color(g, strategy=lambda graph_, colors: order_of(keys).tolist())
    np.testing.assert_array_equal(colour, np.array([ref[v] for v in range(n)], np.uint32))
    assert colour.max() >= 8 and len(sizes) >= 6


def test_model_keys():
    n, seed = 50, 2 ** 64 - 3
    deg = np.arange(n) % 7
    draw = draw_x(seed, np.arange(n, dtype=np.uint64), 0)
    np.testing.assert_array_equal(model_keys(ORDER_RANDOM, seed, n, deg), draw)
    k = model_keys(ORDER_DEGREE, seed, n, deg)
    np.testing.assert_array_equal(k >> np.uint64(32), deg.astype(np.uint64))
    np.testing.assert_array_equal(k & np.uint64(0xFFFFFFFF), draw >> np.uint64(32))
    assert not model_keys(ORDER_ID, seed, n, deg).any()
    np.testing.assert_array_equal(order_of(model_keys(ORDER_ID, seed, n, deg)), np.arange(n))
    o = order_of(k)
    assert np.all(np.diff(deg[o]) <= 0)  # largest degree first
    assert len(np.unique(draw)) == n and not np.array_equal(order_of(draw), np.arange(n))


def test_model_closed_forms():
    # K_12: 12 colours in every order, one member
    i, j = np.triu_indices(12, 1)
    for order in (ORDER_RANDOM, ORDER_DEGREE, ORDER_ID):
        _, _, _, colour, mask, sizes, rounds = both_routes(i, j, 12, order, seed=5)
        assert sorted(colour.tolist()) == list(range(12)) and mask.sum() == 1 and sizes == [1] * 12
        assert rounds["rounds"] == 2 and rounds["members1"] == 1 and rounds["undecided1"] == 11
    # a path on its natural ids under `id`: alternating colours over L levels, the even vertices
    L = 41
    a = np.arange(L - 1)
    _, _, _, colour, mask, sizes, rounds = both_routes(a, a + 1, L, ORDER_ID, seed=0)
    np.testing.assert_array_equal(colour, np.arange(L) % 2)
    np.testing.assert_array_equal(mask, np.arange(L) % 2 == 0)
    assert sizes == [1] * L and rounds["rounds"] == L and rounds["members1"] == 1 and rounds["undecided1"] == L - 1
    # the crown graph on 2 m interleaved vertices (a_i = 2 i, b_j = 2 j + 1, a_i ~ b_j for i != j) under `id`: m colours, where two suffice
    m = 9
    ai, bj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    keep = ai != bj
    u, v = 2 * ai[keep], 2 * bj[keep] + 1
    _, _, _, colour, mask, _, _ = both_routes(np.minimum(u, v), np.maximum(u, v), 2 * m, ORDER_ID, seed=0)
    np.testing.assert_array_equal(colour, np.arange(2 * m) // 2)
    assert mask.sum() == 2
    # no vertices, and vertices without edges
    z = np.zeros(0, np.int64)
    _, _, _, colour, mask, sizes, rounds = both_routes(z, z, 0, ORDER_RANDOM, seed=1)
    assert len(colour) == 0 and sizes == [] and rounds["rounds"] == 0
    _, _, _, colour, mask, sizes, rounds = both_routes(z, z, 7, ORDER_DEGREE, seed=1)
    assert not colour.any() and mask.all() and sizes == [7] and rounds == dict(rounds=1, members1=7, undecided1=0, size=7)


def test_validators_reject():
    a = np.arange(5)
    rows, nbr, keys, rank = graph(a, a + 1, 6, ORDER_ID, 0)
    with pytest.raises(AssertionError):
        assert_proper(rows, nbr, np.array([0, 1, 1, 0, 1, 0]))  # an edge of one colour
    with pytest.raises(AssertionError):
        assert_proper(rows, nbr, np.array([0, 2, 0, 1, 0, 1]))  # colour 2 where 1 was free
    with pytest.raises(AssertionError):
        assert_maximal_independent(rows, nbr, np.array([1, 1, 0, 0, 1, 0], bool))
    with pytest.raises(AssertionError):
        assert_maximal_independent(rows, nbr, np.array([1, 0, 0, 0, 1, 0], bool))  # 2 could join
    assert_proper(rows, nbr, np.array([0, 1, 0, 1, 0, 1]))
    assert_maximal_independent(rows, nbr, np.array([0, 1, 0, 0, 1, 0], bool))
