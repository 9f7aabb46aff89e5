"""CPU only: tests/truss_model.py against networkx.k_truss for every k on a small zoo, and its identities with
triangles_model.model_triangles and kcore_model.model_kcore.  Nothing of the package runs here."""
import numpy as np
import pytest

from kcore_model import model_kcore
from triangles_model import model_triangles
from truss_checks import clique, cylinder, upper
from truss_model import assert_hard, counters_of, hardness, model_support, model_truss


def zoo(streams):
    rng = np.random.default_rng(9)
    out = {}
    out["K9"] = (12, upper(clique(np.arange(1, 10))))
    out["two cliques sharing an edge"] = (20, upper(np.concatenate([clique([1, 2, 3, 4, 5, 6]), clique([1, 2, 10, 11, 12])[1:]])))
    cyc = np.arange(30)
    out["cycle, tree, isolated"] = (90, upper(np.concatenate([np.stack([cyc, np.roll(cyc, -1)], axis=1),
                                                             [[40 + i, 40 + rng.integers(0, i)] for i in range(1, 30)]])))
    out["cylinder"] = (100, upper(cylinder(20, base=3)))
    p = np.arange(2, 42)
    out["book"] = (50, upper(np.concatenate([[[0, 1]], np.stack([np.zeros_like(p), p], axis=1), np.stack([np.ones_like(p), p], axis=1)])))
    s, d = streams.rmat_edges_folded(300, 9, 4000, seed=3)
    rmat = streams.adds(s, d)
    out["rmat, both orientations, loops, beyond"] = (300, np.concatenate([rmat, rmat[::3, [1, 0, 2]], [[7, 7, 1], [8, 400, 1]]]).astype(np.uint32))
    out["empty"] = (5, np.zeros((0, 3), np.uint32))
    return out


def stored(ops):
    """the distinct stored pairs of a stream of adds"""
    key = np.unique(ops[:, 0].astype(np.int64) << 32 | ops[:, 1].astype(np.int64))
    return key >> 32, key & 0xFFFFFFFF


def test_truss_model_closed_forms(streams):
    z = zoo(streams)
    mt = model_truss(*stored(z["K9"][1]), 12)
    assert np.all(mt["support"] == 7) and np.all(mt["truss"] == 9) and counters_of(mt) == [36, 84, 1, 1, 1, 36]
    mt = model_truss(*stored(z["two cliques sharing an edge"][1]), 20)
    t = {(a, b): k for a, b, k in zip(mt["a"].tolist(), mt["b"].tolist(), mt["truss"].tolist())}
    assert t[1, 2] == 6 and t[3, 6] == 6 and t[1, 10] == 5 and t[10, 12] == 5 and sorted(set(t.values())) == [5, 6]
    mt = model_truss(*stored(z["cycle, tree, isolated"][1]), 90)
    assert np.all(mt["truss"] == 2) and mt["total"] == 0 and mt["subrounds"] == [1] and not mt["vtruss"][70:].any()
    mt = model_truss(*stored(z["cylinder"][1]), 100)
    assert np.all(mt["truss"] == 3) and mt["levels"] == 1 and mt["subrounds"] == [20] and mt["widest"] <= 16
    mt = model_truss(*stored(z["book"][1]), 50)
    assert mt["support"][0] == 40 and np.all(mt["truss"] == 3) and mt["subrounds"] == [2] and mt["widest"] == 80
    mt = model_truss(*stored(z["empty"][1]), 5)
    assert counters_of(mt) == [0, 0, 0, 0, 0, 0] and mt["tmax"] == 0 and not mt["vtruss"].any()


def test_truss_model_against_networkx(streams):
    """k_truss(G, k) is the subgraph of the edges with truss >= k, for every k up to tmax + 1"""
    nx = pytest.importorskip("networkx")
    for name, (n, ops) in zoo(streams).items():
        src, dst = stored(ops)
        mt = model_truss(src, dst, n)
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from(zip(mt["a"].tolist(), mt["b"].tolist()))
        for k in range(2, mt["tmax"] + 2):
            ref = {(min(x, y), max(x, y)) for x, y in nx.k_truss(g, k).edges()}
            keep = mt["truss"] >= k
            assert ref == set(zip(mt["a"][keep].tolist(), mt["b"][keep].tolist())), (name, k)
        tri = nx.triangles(g)
        assert sum(tri.values()) == 3 * mt["total"], name


def test_truss_model_identities(streams):
    """supports sum to 3 x the triangles and, per vertex, to 2 x tri[v]; vtruss <= core + 1; what hardness() reports"""
    for name, (n, ops) in zoo(streams).items():
        src, dst = stored(ops)
        a, b, sup, total = model_support(src, dst, n)
        tri, want_total = model_triangles(src, dst, n)
        assert total == want_total and int(sup.sum()) == 3 * total, name
        at = np.bincount(a, weights=sup, minlength=n) + np.bincount(b, weights=sup, minlength=n)
        np.testing.assert_array_equal(at.astype(np.uint64), 2 * tri, err_msg=name)
        mt = model_truss(src, dst, n)
        core = model_kcore(src, dst, n)
        assert np.all(mt["vtruss"] <= core + 1) and mt["tmax"] <= (int(core.max()) if n else 0) + 1, name
        assert np.all(mt["truss"] <= mt["support"] + 2) and np.all(mt["truss"] >= 2), name
    n, ops = zoo(streams)["rmat, both orientations, loops, beyond"]
    src, dst = stored(ops)
    mt = model_truss(src, dst, n)
    h = hardness(src, dst, n, mt, firsts=[0, 100, 200])
    assert_hard(h, "rmat", tmax=5, distinct=4, below_support=50, max_support=10, backward=100, loops=1, beyond=1, cross=100, max_subrounds=2)
    with pytest.raises(AssertionError):
        assert_hard(h, "rmat", tmax=h["tmax"] + 1)
