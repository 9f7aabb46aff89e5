"""CPU: pppcsr_bfs / pppcsr_pagerank (the reference's bfs.h / pagerank.h templates with T = PPPCSR) on the fiber SIMT emulator
(tests/hostsim), which compiles the engine's own kernel and host source.  Results are checked against a numpy model of the
templates built from the exported partition states (tests/consumers_model.py): levels equal, PageRank byte for byte."""
import ctypes

import numpy as np
import pytest

from consumers_model import global_edges, last_slot_free, model_bfs, model_pagerank, num_neighbors, partition_states
from helpers import digest, load_pkg
from test_sim_engine import SIM_SO, build_sim

EINVAL = 1


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


def tune(pp):
    """emulator-sized scheduler options on every partition (a repartition recreates the engines: call again after it)"""
    for k in range(pp.num_partitions()):
        e = pp.partition(k)
        for key, v in dict(mode=1, opt_horizon=64, epoch_ops=1024, region_slots=64, small_batch=0, big_grid=2, big_min=512,
                           big_window=131072, max_horizon=32, min_horizon=4, init_horizon=8, rounds_per_sync=2).items():
            e.set_option(key, v)


def make(lib, n, P):
    pp = load_pkg().PPPCSR(n, numDomain=1, partitionsPerDomain=P, lib=lib)
    tune(pp)
    return pp


def values(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 64, n) / 8.0).astype(np.float32)  # (strictly positive: no 0 / 0)


def mixed_stream(streams, n, seed):
    """random and RMAT adds, deletes (mostly of missing edges), duplicate adds, destinations >= n, and a vertex whose
    num_neighbors wraps below zero"""
    a = streams.random_stream(n, 1500, seed=seed, p_delete=0.25)
    s, d = streams.rmat_edges_folded(n, 11, 1500, seed=seed + 1)
    b = streams.adds(s, d)
    ops = np.concatenate([a, b, b[::5]])  # (b[::5]: duplicates)
    ops[::17, 1] += np.uint32(n)  # destinations beyond the graph
    ops = ops[np.random.default_rng(seed).permutation(len(ops))]
    lone = n // 2 + 1  # deletes on a vertex with no edges: num_neighbors 0 - 2 wraps
    ops = ops[ops[:, 0] != lone]
    return np.concatenate([ops, np.array([[lone, 1, 0], [lone, 2, 0]], np.uint32)])


def check(pp, starts, vals, label, want_wide=False):
    """levels and PageRank against the model; nothing written (states and stats)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    widest = 0
    for s in starts:
        ref, w = model_bfs(src, dst, n, s)
        widest = max(widest, w)
        np.testing.assert_array_equal(pp.bfs(s), ref, err_msg=f"{label}: bfs from {s}")
    if want_wide:  # a frontier at or above the streaming pass's threshold was met
        assert widest >= max(64, n // 256), (label, widest)
    got = pp.pagerank(vals)
    ref = model_pagerank(src, dst, num_neighbors(states), vals)
    assert got.tobytes() == ref.tobytes(), f"{label}: pagerank differs at {np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0][:10]}"
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return got


def starts_of(pp, isolated):
    P, n = pp.num_partitions(), pp.get_n()
    mid = pp.partition_start(P // 2) + 3 if P > 1 else n // 2
    return [0, int(mid), n - 2, isolated]


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_pppcsr_consumers_model(lib, streams, P):
    """mixed streams, add_node, then pppcsr_repartition to balanced_starts; a second graph with a hub the per-vertex kernel
    defers, bulk-built"""
    n = 1200
    pp = make(lib, n, P)
    ops = mixed_stream(streams, n, seed=40 + P)
    pp.apply(ops[: len(ops) // 2])
    pp.apply(ops[len(ops) // 2:])
    pp.add_node()
    pp.add_node()
    pp.apply(np.array([[n, 3, 1], [n, 5, 1], [7, n, 1], [n + 5, 1, 1]], np.uint32))  # vertex n + 1 stays isolated
    vals = values(n + 2, seed=P)
    check(pp, starts_of(pp, n + 1), vals, f"P={P}", want_wide=True)
    pp.repartition(pp.balanced_starts())
    tune(pp)
    check(pp, starts_of(pp, n + 1), vals, f"P={P} repartitioned")
    pp.close()

    hub = 3 if P == 1 else 2 * n // P + 1
    m = 5000
    rng = np.random.default_rng(P)
    adds = np.concatenate([streams.adds(np.full(m, hub, np.uint32), rng.permutation(m + 500)[:m].astype(np.uint32)),
                           streams.adds(*streams.rmat_edges_folded(n, 11, 2000, seed=9))])
    pp = make(lib, n, P)
    pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
    node = pp.getNode(hub)
    assert node[1] - node[0] > 4096
    check(pp, [hub, 0, n - 1, int(adds[-1, 1])], values(n, seed=7), f"P={P} hub")
    pp.apply(streams.random_stream(n, 500, seed=3, p_delete=0.3))
    check(pp, [hub, 1], values(n, seed=8), f"P={P} hub + stream")


def test_sim_pppcsr_consumers_invariant(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and one graph before and after a repartition: equal levels, bitwise-equal PageRank"""
    n = 1000
    ops = mixed_stream(streams, n, seed=5)
    vals = values(n, seed=5)
    starts = [0, 333, 999, n // 2 + 1]
    results = []
    for P in (1, 2, 4, 8):
        pp = make(lib, n, P)
        pp.apply(ops)
        assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
        results.append(([pp.bfs(s) for s in starts], pp.pagerank(vals)))
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
            assert all(last_slot_free(i) for _, i, _ in partition_states(pp))
            results.append(([pp.bfs(s) for s in starts], pp.pagerank(vals)))
        pp.close()
    for lv, pr in results[1:]:
        for a, b in zip(lv, results[0][0]):
            np.testing.assert_array_equal(a, b)
        assert pr.tobytes() == results[0][1].tobytes()


def test_sim_pppcsr_consumers_one_partition_is_the_engine(lib, streams):
    """P = 1: the results of ppcsr_bfs / ppcsr_pagerank on the partition's own engine"""
    n = 700
    pp = make(lib, n, 1)
    pp.apply(mixed_stream(streams, n, seed=11))
    e = pp.partition(0)
    vals = values(n, seed=11)
    for s in (0, 350, n - 1):
        np.testing.assert_array_equal(pp.bfs(s), e.bfs(s))
    assert pp.pagerank(vals).tobytes() == e.pagerank(vals).tobytes()


def test_sim_pppcsr_consumers_write_nothing(lib, streams):
    """after the calls every partition is what OraclePPPCSR holds, and a following batch still matches it"""
    from oracle_lib import OraclePPPCSR
    n, P = 800, 4
    pp, o = make(lib, n, P), OraclePPPCSR(n, True, 1, P)
    a = streams.random_stream(n, 2500, seed=2, p_delete=0.2)
    b = streams.random_stream(n, 1500, seed=3, p_delete=0.3)
    pp.apply(a)
    o.apply(a)

    def same(label):
        for k in range(P):
            x, y = pp.partition(k), o.partition(k)
            assert digest(*x.state(), x.geometry()) == digest(*y.state(), y.geometry()), f"{label}: partition {k}"

    same("before")
    check(pp, [0, 401, n - 1], values(n, seed=2), "P=4")
    same("after the calls")
    pp.apply(b)
    o.apply(b)
    same("after the next batch")


def test_sim_pppcsr_consumers_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    pp.apply(streams.random_stream(n, 500, seed=1))
    L, h = pp.L, pp.h
    lv = np.empty(n, np.uint32)
    vals = np.ones(n, np.float32)
    out = np.empty(n, np.float32)
    ms = ctypes.c_double()
    assert L.pppcsr_bfs(h, n, lv.ctypes.data, ctypes.byref(ms)) == EINVAL
    assert L.pppcsr_bfs(h, 0xFFFFFFFF, lv.ctypes.data, None) == EINVAL
    assert L.pppcsr_bfs(h, 0, None, None) == EINVAL
    assert L.pppcsr_bfs(None, 0, lv.ctypes.data, None) == EINVAL
    assert L.pppcsr_pagerank(h, None, out.ctypes.data, None) == EINVAL
    assert L.pppcsr_pagerank(h, vals.ctypes.data, None, None) == EINVAL
    assert L.pppcsr_pagerank(None, vals.ctypes.data, out.ctypes.data, None) == EINVAL
    assert L.pppcsr_bfs(h, n - 1, lv.ctypes.data, None) == 0  # device_ms may be NULL
    assert L.pppcsr_pagerank(h, vals.ctypes.data, out.ctypes.data, None) == 0
    with pytest.raises(pkg.PpcsrError):
        pp.bfs(n)
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_bfs(loc.h, 100, lv.ctypes.data, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_pagerank(loc.h, vals.ctypes.data, out.ctypes.data, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED — partitions on several devices — needs a second device: the emulator has one)
