"""CPU: tests/multibfs_model.py itself — its rows against consumers_model.model_bfs and the levels recorded from the reference's
bfs.h on a fixture, and its aggregates on three graphs computed by hand."""
import numpy as np

from consumers_model import NO_LEVEL, model_bfs
from helpers import golden
from multibfs_model import aggregates, hist_of, model_multi_bfs


def edges_of(ops):
    """the edge set a stream leaves behind (value 0 deletes), ascending (src, dst)"""
    live = {}
    for s, d, v in ops.tolist():
        if v:
            live[(s, d)] = v
        else:
            live.pop((s, d), None)
    e = np.array(sorted(live), np.int64).reshape(-1, 2)
    return e[:, 0], e[:, 1]


def test_model_rows_equal_model_bfs_on_the_fixture():
    g = golden("consumers_rmat12")
    n = int(g["n"])
    src, dst = edges_of(g["ops"])
    rng = np.random.default_rng(1)
    sources = np.concatenate([g["starts"], rng.integers(0, n, 20), g["starts"][:1]]).astype(np.uint32)
    m = model_multi_bfs(src, dst, n, sources)
    for i, s in enumerate(sources):
        want, _ = model_bfs(src, dst, n, int(s))
        np.testing.assert_array_equal(m["levels"][i], want)
        assert aggregates(hist_of(want)) == (m["reached"][i], m["far"][i], m["ecc"][i], m["harmonic"][i])
        assert hist_of(want) == m["hists"][i]
    np.testing.assert_array_equal(m["levels"][: len(g["starts"])], g["levels"])  # (recorded from the reference's queue walk)
    assert max(m["ecc"]) >= 3 and max(m["reached"]) > n // 2


def test_model_path():
    """0 -> 1 -> ... -> 9: from 0 every level holds one vertex; from 7 two remain; from 9 nothing"""
    n = 10
    src, dst = np.arange(9), np.arange(1, 10)
    m = model_multi_bfs(src, dst, n, [0, 7, 9, 0])
    assert m["reached"] == [10, 3, 1, 10]
    assert m["far"] == [45, 3, 0, 45]
    assert m["ecc"] == [9, 2, 0, 9]
    h = 0.0
    for L in range(1, 10):
        h += 1.0 / L
    assert m["harmonic"].tolist() == [h, 1.5, 0.0, h]
    np.testing.assert_array_equal(m["levels"][0], np.arange(10))
    np.testing.assert_array_equal(m["levels"][1], [NO_LEVEL] * 7 + [0, 1, 2])
    np.testing.assert_array_equal(m["levels"][2], [NO_LEVEL] * 9 + [0])


def test_model_star():
    """centre 0 -> 1 .. 6, a leaf has no way back; an edge to a destination >= n and a self-loop count for nothing"""
    n = 7
    src = np.array([0] * 6 + [0, 3])
    dst = np.array([1, 2, 3, 4, 5, 6] + [n + 2, 3])
    m = model_multi_bfs(src, dst, n, [0, 3])
    assert m["reached"] == [7, 1] and m["far"] == [6, 0] and m["ecc"] == [1, 0]
    assert m["harmonic"].tolist() == [6.0, 0.0]
    np.testing.assert_array_equal(m["levels"][0], [0, 1, 1, 1, 1, 1, 1])


def test_model_two_components():
    """a directed triangle 0 -> 1 -> 2 -> 0 and, apart from it, 3 -> 4, 3 -> 5, 4 -> 5; 6 is isolated"""
    n = 7
    src = np.array([0, 1, 2, 3, 3, 4])
    dst = np.array([1, 2, 0, 4, 5, 5])
    m = model_multi_bfs(src, dst, n, [0, 3, 4, 6, 2])
    assert m["reached"] == [3, 3, 2, 1, 3]
    assert m["far"] == [3, 2, 1, 0, 3]
    assert m["ecc"] == [2, 1, 1, 0, 2]
    assert m["harmonic"].tolist() == [1.0 + 1.0 / 2.0, 2.0, 1.0, 0.0, 1.5]
    np.testing.assert_array_equal(m["levels"][4], [1, 2, 0, NO_LEVEL, NO_LEVEL, NO_LEVEL, NO_LEVEL])
