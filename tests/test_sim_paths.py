"""CPU: ppcsr_sssp / ppcsr_components and their pppcsr_ forms on the fiber SIMT emulator (tests/hostsim), which compiles the
engine's own kernel and host source.  Results are checked exactly against tests/paths_model.py (heap Dijkstra on Python
integers, union-find to the smallest id), built from the exported partition states."""
import ctypes

import numpy as np
import pytest

from consumers_model import global_edges, last_slot_free, model_bfs, partition_states
from helpers import load_pkg
from paths_model import (NO_PATH, assert_hard, global_edges_valued, hardness, levels_as_dist, model_components, model_sssp)
from test_sim_engine import SIM_SO, build_sim
from test_sim_pppcsr_consumers import make, mixed_stream, starts_of, tune

EINVAL = 1


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


def weigh(streams, ops, hi, seed):
    """the adds of `ops` with values in [1, hi] from the counter hash (one counter per row: a duplicate add changes the value)"""
    ops = ops.copy()
    w = (streams.uniform_ints(seed, len(ops), hi) + 1).astype(np.uint32)
    add = ops[:, 2] != 0
    ops[add, 2] = w[add]
    return ops


def replay(ops_list, n_src):
    """{(src, dst): value} after the ops in order: the last add of a pair wins, a delete removes it"""
    held = {}
    for ops in ops_list:
        for s, d, v in ops.tolist():
            if s >= n_src:
                continue
            if v:
                held[(s, d)] = v
            else:
                held.pop((s, d), None)
    return held


def check(pp, starts, label, hard_start=None):
    """sssp from every start and components against the model; nothing written (states and stats)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst, val = global_edges_valued(states)
    if hard_start is not None:
        lv, widest = model_bfs(src, dst, n, hard_start)
        h, _ = hardness(src, dst, val, n, hard_start, lv, widest)
        assert_hard(h, n, label)
    for s in starts:
        np.testing.assert_array_equal(pp.sssp(s), model_sssp(src, dst, val, n, s), err_msg=f"{label}: sssp from {s}")
    np.testing.assert_array_equal(pp.components(), model_components(src, dst, n), err_msg=f"{label}: components")
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return src, dst, val


@pytest.mark.parametrize("hi", [1000, 4])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_paths_model(lib, streams, P, hi):
    """mixed weighted streams (deletes, duplicate adds with new values, destinations >= n), add_node, a repartition to
    balanced_starts; then a bulk-built graph with a hub the per-vertex kernel defers.  hi = 4: many paths of equal length"""
    n = 1200
    pp = make(lib, n, P)
    ops = weigh(streams, mixed_stream(streams, n, seed=40 + P), hi, seed=7 * P + hi)
    tail = np.array([[n, 3, 2], [n, 5, 1], [7, n, 3], [n + 5, 1, 1]], np.uint32)  # vertex n + 1 stays isolated
    pp.apply(ops[: len(ops) // 2])
    pp.apply(ops[len(ops) // 2:])
    pp.add_node()
    pp.add_node()
    pp.apply(tail)
    main = int(ops[np.nonzero(ops[:, 2])[0][0], 0])  # the source of an edge
    src, dst, val = check(pp, starts_of(pp, n + 1) + seams(pp) + [main, n], f"P={P} hi={hi}", hard_start=_best_start(pp))
    # the last add of a pair won (the model above is built from the stored values: this ties them to the stream)
    held = replay([ops], n)
    held.update(replay([tail], n + 2))
    assert dict(zip(zip(src.tolist(), dst.tolist()), val.tolist())) == held
    pp.repartition(pp.balanced_starts())
    tune(pp)
    check(pp, starts_of(pp, n + 1) + seams(pp) + [main], f"P={P} hi={hi} repartitioned")
    pp.close()

    hub = 3 if P == 1 else 2 * n // P + 1
    m = 5000
    rng = np.random.default_rng(P)
    adds = np.concatenate([streams.adds(np.full(m, hub, np.uint32), rng.permutation(m + 500)[:m].astype(np.uint32)),
                           streams.adds(*streams.rmat_edges_folded(n, 11, 2000, seed=9))])
    adds = weigh(streams, adds, hi, seed=3)
    pp = make(lib, n, P)
    pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
    node = pp.getNode(hub)
    assert node[1] - node[0] > 4096
    check(pp, [hub, 0, n - 1, int(adds[-1, 0])], f"P={P} hi={hi} hub")
    pp.apply(weigh(streams, streams.random_stream(n, 500, seed=3, p_delete=0.3), hi, seed=4))
    check(pp, [hub, 1], f"P={P} hi={hi} hub + stream")


def seams(pp):
    """the first vertex of a partition in the middle and the last vertex of the one before it"""
    if pp.num_partitions() == 1:
        return []
    first = int(pp.partition_start(pp.num_partitions() // 2))
    return [first, first - 1]


def _best_start(pp):
    """the start the three model conditions are asserted from: the vertex of largest out-degree (reaches the giant component)"""
    states = partition_states(pp)
    src, dst = global_edges(states)
    return int(np.bincount(src[dst < pp.get_n()]).argmax())


def test_sim_paths_conditions_on_the_issue_graph(lib, streams):
    """the plain folded RMAT graph with values in [1, 1000] and in [1, 4]: the three conditions hold from the model, and the
    device equals the model — with every wv::uni / wv::bcast of the kernels verified"""
    n = 1200
    s, d = streams.rmat_edges_folded(n, 11, 3000, seed=41)
    lib.ppcsr_sim_check_uniform(1)
    try:
        for hi in (1000, 4):
            pp = make(lib, n, 3)
            pp.apply(weigh(streams, streams.adds(s, d), hi, seed=hi))
            start = _best_start(pp)
            src, dst, val = check(pp, [start, 0, n - 1], f"hi={hi}", hard_start=start)
            np.testing.assert_array_equal(pp.bfs(start), model_bfs(src, dst, n, start)[0])
            pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


def test_sim_sssp_64_bit_distances(lib):
    """5 edges of value 0xFFFFFFFE add up beyond 2^32; a value-1 edge from an unreachable vertex must not win"""
    big = 0xFFFFFFFE
    for P in (1, 3):
        pp = make(lib, 40, P)
        path = [0, 17, 5, 33, 9, 21]
        ops = [[a, b, big] for a, b in zip(path, path[1:])] + [[30, 21, 1], [30, 9, 1], [21, 2, 7]]
        pp.apply(np.array(ops, np.uint32))
        dist = pp.sssp(0)
        for k, v in enumerate(path):
            assert int(dist[v]) == k * big
        assert int(dist[21]) == 5 * (2 ** 32 - 2) and int(dist[2]) == 5 * big + 7
        assert int(dist[30]) == NO_PATH
        src, dst, val = global_edges_valued(partition_states(pp))
        np.testing.assert_array_equal(dist, model_sssp(src, dst, val, 40, 0))
        assert int(pp.sssp(30)[21]) == 1
        pp.close()


@pytest.mark.parametrize("P", [1, 4])
def test_sim_paths_many_rounds(lib, P):
    """a path over 600 permuted vertices with values 1-3 must beat shortcuts of value 10^6 to every 50th of its vertices;
    40 disjoint directed cycles.  The path is one component that needs repeated hook and jump rounds"""
    n, L = 1000, 600
    rng = np.random.default_rng(12)
    perm = rng.permutation(n)
    path, rest = perm[:L], perm[L:]
    w = rng.integers(1, 4, L - 1)
    ops = [[int(a), int(b), int(x)] for a, b, x in zip(path, path[1:], w)]
    ops += [[int(path[0]), int(path[k]), 10 ** 6] for k in range(50, L, 50)]
    cycles = rest[:400].reshape(40, 10)
    for c in cycles:
        ops += [[int(a), int(b), 2] for a, b in zip(c, np.roll(c, -1))]
    ops = np.array(ops, np.uint32)
    pp = make(lib, n, P)
    pp.apply(ops[rng.permutation(len(ops))])
    dist = pp.sssp(int(path[0]))
    want = np.concatenate([[0], np.cumsum(w)])
    np.testing.assert_array_equal(dist[path], want.astype(np.uint64))
    assert want[-1] < 10 ** 6  # (every shortcut loses)
    assert np.all(dist[rest] == np.uint64(NO_PATH))
    labels = pp.components()
    assert np.all(labels[path] == path.min())
    for c in cycles:
        assert np.all(labels[c] == c.min())
        dc = pp.sssp(int(c[3]))
        np.testing.assert_array_equal(dc[np.roll(c, -3)], 2 * np.arange(10, dtype=np.uint64))
    lone = rest[400:]
    np.testing.assert_array_equal(labels[lone], lone.astype(np.uint32))
    src, dst, val = global_edges_valued(partition_states(pp))
    np.testing.assert_array_equal(labels, model_components(src, dst, n))
    np.testing.assert_array_equal(dist, model_sssp(src, dst, val, n, int(path[0])))
    pp.close()


def test_sim_paths_direction(lib):
    """only a -> b: no path from b to a, one component"""
    pp = make(lib, 20, 2)
    a, b = 13, 4
    pp.apply(np.array([[a, b, 5]], np.uint32))
    assert int(pp.sssp(b)[a]) == NO_PATH and int(pp.sssp(a)[b]) == 5
    labels = pp.components()
    assert labels[a] == labels[b] == b
    want = np.arange(20, dtype=np.uint32)
    want[a] = b
    np.testing.assert_array_equal(labels, want)
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_sssp_unit_values_is_bfs(lib, streams, P):
    n = 900
    pp = make(lib, n, P)
    ops = mixed_stream(streams, n, seed=21)  # (every add has value 1)
    pp.apply(ops)
    for s in (0, 450, n - 1, int(ops[0, 0]), _best_start(pp)):
        np.testing.assert_array_equal(pp.sssp(s), levels_as_dist(pp.bfs(s)))
    pp.close()


def test_sim_paths_invariant(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and one graph before and after a repartition with an empty partition: equal results;
    P = 1 equals the partition's own engine calls"""
    n = 1000
    ops = weigh(streams, mixed_stream(streams, n, seed=5), 50, seed=5)
    starts = [0, 333, 999, n // 2 + 1, int(ops[0, 0])]
    results = []
    for P in (1, 2, 4, 8):
        pp = make(lib, n, P)
        pp.apply(ops)
        assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
        results.append(([pp.sssp(s) for s in starts], pp.components()))
        if P == 1:
            e = pp.partition(0)
            for s, got in zip(starts, results[0][0]):
                np.testing.assert_array_equal(e.sssp(s), got)
            np.testing.assert_array_equal(e.components(), results[0][1])
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
            tune(pp)
            assert all(last_slot_free(i) for _, i, _ in partition_states(pp))
            results.append(([pp.sssp(s) for s in starts], pp.components()))
        pp.close()
    assert len(np.unique(results[0][1])) > 1 and np.count_nonzero(results[0][0][-1] != np.uint64(NO_PATH)) > n // 4
    for ds, lab in results[1:]:
        for a, b in zip(ds, results[0][0]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(lab, results[0][1])


def test_paths_model_against_scipy(lib, streams):
    """the model itself against scipy.sparse.csgraph on a small graph"""
    sp = pytest.importorskip("scipy.sparse")
    cg = pytest.importorskip("scipy.sparse.csgraph")
    n = 600
    pp = make(lib, n, 3)
    pp.apply(weigh(streams, mixed_stream(streams, n, seed=8), 1000, seed=8))
    src, dst, val = global_edges_valued(partition_states(pp))
    ok = dst < n
    g = sp.csr_matrix((val[ok].astype(np.float64), (src[ok], dst[ok])), shape=(n, n))  # (pairs are unique: nothing is summed)
    for s in (0, 299, int(src[0])):
        ref = cg.dijkstra(g, directed=True, indices=s)
        want = np.where(np.isinf(ref), float(NO_PATH), ref)
        got = model_sssp(src, dst, val, n, s)
        assert np.array_equal(got == np.uint64(NO_PATH), np.isinf(ref))
        assert np.array_equal(got[~np.isinf(ref)], want[~np.isinf(ref)].astype(np.uint64))
        np.testing.assert_array_equal(pp.sssp(s), got)
    _, comp = cg.connected_components(g, directed=True, connection="weak")
    smallest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))  # scipy's labels are arbitrary: map every component to its smallest id
    np.testing.assert_array_equal(model_components(src, dst, n), smallest[comp].astype(np.uint32))
    pp.close()


def test_sim_paths_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    pp.apply(streams.random_stream(n, 500, seed=1))
    L, h = pp.L, pp.h
    dist = np.empty(n, np.uint64)
    lab = np.empty(n, np.uint32)
    ms = ctypes.c_double()
    assert L.pppcsr_sssp(h, n, dist.ctypes.data, ctypes.byref(ms)) == EINVAL
    assert L.pppcsr_sssp(h, 0xFFFFFFFF, dist.ctypes.data, None) == EINVAL
    assert L.pppcsr_sssp(h, 0, None, None) == EINVAL
    assert L.pppcsr_sssp(None, 0, dist.ctypes.data, None) == EINVAL
    assert L.pppcsr_components(h, None, None) == EINVAL
    assert L.pppcsr_components(None, lab.ctypes.data, None) == EINVAL
    assert L.pppcsr_sssp(h, n - 1, dist.ctypes.data, None) == 0  # device_ms may be NULL
    assert L.pppcsr_components(h, lab.ctypes.data, None) == 0
    assert L.pppcsr_sssp(h, 0, dist.ctypes.data, ctypes.byref(ms)) == 0 and ms.value >= 0.0
    e = pp.partition(0)
    m = e.get_n()
    assert L.ppcsr_sssp(e.h, m, dist.ctypes.data, None) == EINVAL
    assert L.ppcsr_sssp(e.h, 0, None, None) == EINVAL
    assert L.ppcsr_sssp(None, 0, dist.ctypes.data, None) == EINVAL
    assert L.ppcsr_components(e.h, None, None) == EINVAL
    assert L.ppcsr_components(None, lab.ctypes.data, None) == EINVAL
    assert L.ppcsr_sssp(e.h, m - 1, dist.ctypes.data, None) == 0
    assert L.ppcsr_components(e.h, lab.ctypes.data, None) == 0
    with pytest.raises(pkg.PpcsrError):
        pp.sssp(n)
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_sssp(loc.h, 100, dist.ctypes.data, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_components(loc.h, lab.ctypes.data, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED — partitions on several devices — needs a second device: the emulator has one)
