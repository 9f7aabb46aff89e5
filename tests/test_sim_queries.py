"""CPU: the batched reads (ppcsr_lookup_edges / ppcsr_gather_neighbourhoods and the PPPCSR forms) on the fiber SIMT
emulator (tests/hostsim), which compiles the engine's own kernel and host source.  States are built by replaying golden
fixtures, checked bit-identical to the oracle, and then queried: existence against Oracle.edge_exists and the engine's own
single call, values against the exported slots, gathered rows against Oracle.get_neighbourhood."""
import ctypes

import numpy as np
import pytest

from helpers import golden, load_pkg
from oracle_lib import Oracle
from test_sim_engine import SIM_SO, build_sim

NO_EDGE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


def make(lib, n, lock=True):
    e = load_pkg().PCSR(n, lock_search=lock, lib=lib)
    for k, v in [("mode", 0), ("max_horizon", 32), ("min_horizon", 4), ("init_horizon", 8), ("rounds_per_sync", 2), ("small_batch", 0),
                 ("big_grid", 2), ("big_min", 512), ("big_window", 131072)]:
        e.set_option(k, v)
    return e


def same_state(e, o, label=""):
    assert e.geometry() == o.geometry(), label
    ei, en = e.state()
    oi, on = o.state()
    np.testing.assert_array_equal(en, on, err_msg=label + " nodes")
    np.testing.assert_array_equal(ei, oi, err_msg=label + " items")


def live_slots(items, nodes, v):
    """live slots of (beginning, end) of v in slot order: what get_neighbourhood reads (PCSR.cpp:901-912)"""
    if v >= len(nodes):
        return np.empty((0, 3), np.uint32)
    b, e = int(nodes[v][0]), int(nodes[v][1])
    s = items[b + 1:e] if e > b + 1 else items[0:0]
    return s[s[:, 2] != 0]


def make_queries(rng, items, nodes, ops, m):
    n = len(nodes)
    live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)
    present = items[live][:, :2]
    parts = []
    if len(present):
        parts.append(present[rng.integers(0, len(present), m // 3)])
    dele = ops[ops[:, 2] == 0][:, :2] if len(ops) else np.empty((0, 2), np.uint32)
    if len(dele):
        parts.append(dele[rng.integers(0, len(dele), m // 6)])
    hi = max(n, 1)
    parts.append(np.stack([rng.integers(0, hi, m // 6), rng.integers(0, 4 * hi, m // 6)], 1))  # mostly never present
    parts.append(np.stack([rng.integers(n, n + 1000, m // 20), rng.integers(0, hi, m // 20)], 1))  # src >= n
    parts.append(np.array([[n + 5, 0], [0xFFFFFFFF, 1], [0xFFFFFFFF, 0xFFFFFFFF]]))
    parts.append(np.stack([rng.integers(0, hi, m // 20), np.zeros(m // 20, np.int64)], 1))  # dst = 0
    parts.append(np.stack([rng.integers(0, hi, m // 20), np.full(m // 20, 0xFFFFFFFF)], 1))  # the sentinel dest
    q = np.concatenate([p.astype(np.uint32) for p in parts])
    q = np.concatenate([q, q[rng.integers(0, len(q), m // 10)]])  # repeated pairs
    return q[rng.permutation(len(q))]


def check_state(e, o, ops, rng, m=20000, sample=150):
    """queries against the oracle / the engine's single calls on the state e holds; e's state must not change"""
    same_state(e, o)
    items, nodes = e.state()
    st0 = e.stats()
    n = len(nodes)
    sorted_regime = st0["narrow"] == 1
    q = make_queries(rng, items, nodes, ops, m)
    vals = e.lookup_edges(q[:, 0], q[:, 1])
    exist = np.array([(int(s) < n and o.edge_exists(int(s), int(d))) for s, d in q])
    np.testing.assert_array_equal(vals != NO_EDGE, exist)
    np.testing.assert_array_equal(e.edges_exist(q[:, 0], q[:, 1]), exist)
    assert not np.any(exist & (q[:, 1] == 0xFFFFFFFF))
    for j in rng.choice(len(q), min(sample, len(q)), replace=False):  # the engine's own single call
        s, d = int(q[j, 0]), int(q[j, 1])
        if s < n:
            assert e.edge_exists(s, d) == (vals[j] != NO_EDGE), (s, d)
    if sorted_regime:  # one live slot per edge: its value
        live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)
        table = {(int(s), int(d)): int(v) for s, d, v in items[live]}
        for j in np.nonzero(exist)[0]:
            assert vals[j] == table[(int(q[j, 0]), int(q[j, 1]))]
    # gathers: every vertex, out-of-range ones, repeats, shuffled
    verts = np.concatenate([np.arange(n), np.arange(n, n + 7), np.array([0xFFFFFFFF]), rng.integers(0, max(n, 1), 50)]).astype(np.uint32)
    verts = verts[rng.permutation(len(verts))]
    rows, dests, gv = e.gather_neighbourhoods(verts)
    assert rows[0] == 0 and rows[-1] == len(dests) == len(gv)
    for i, v in enumerate(verts):
        a, b = int(rows[i]), int(rows[i + 1])
        sl = live_slots(items, nodes, int(v))
        ref = o.get_neighbourhood(int(v)) if v < n else np.empty(0, np.int32)
        np.testing.assert_array_equal(dests[a:b], ref, err_msg=f"row of {v}")
        np.testing.assert_array_equal(dests[a:b], sl[:, 1].astype(np.int32), err_msg=f"row of {v}")
        np.testing.assert_array_equal(gv[a:b], sl[:, 2], err_msg=f"values of {v}")
    r2, d2, v2 = e.gather_neighbourhoods(verts, with_values=False)
    assert v2 is None
    np.testing.assert_array_equal(r2, rows)
    np.testing.assert_array_equal(d2, dests)
    # nothing written
    i1, n1 = e.state()
    np.testing.assert_array_equal(i1, items)
    np.testing.assert_array_equal(n1, nodes)
    assert e.stats() == st0


def replay_checked(lib, name, rng, every=1, m=20000):
    g = golden(name)
    n, lock = int(g["n"]), bool(int(g["lock_search"]))
    e, o = make(lib, n, lock), Oracle(n, lock_search=lock)
    if name == "add_node_empty_then_edges":
        for _ in range(5):
            e.add_node()
            o.add_node()
    ops, cps = g["ops"], g["checkpoints"]
    prev = 0
    for i, c in enumerate(cps):
        e.apply(ops[prev:c])
        o.apply(ops[prev:c])
        prev = int(c)
        if i % every == 0 or i == len(cps) - 1:
            check_state(e, o, ops[:prev], rng, m=m)
    return e, o


@pytest.mark.parametrize("name,every", [("random_2e4_n1000", 1000), ("hub_1e4_insert_then_delete", 1), ("add_node_empty_then_edges", 1)])
def test_sim_queries_on_golden_states(lib, name, every):
    replay_checked(lib, name, np.random.default_rng(sum(name.encode())), every=every)


def test_sim_queries_across_doubling_and_halving(lib):
    """dense_n40_grow_shrink: queried at every checkpoint while the array doubles and halves"""
    g = golden("dense_n40_grow_shrink")
    geoms = {tuple(int(x) for x in gg) for gg in g["geoms"]}
    assert len({gg[0] for gg in geoms}) >= 3  # (several array sizes among the checkpoints)
    replay_checked(lib, "dense_n40_grow_shrink", np.random.default_rng(4), every=1, m=4000)


def test_sim_queries_literal_walk_regime(lib, streams):
    """narrow == 0: the search is the reference's literal walk (forced as in test_sim_engine.py)"""
    ops = streams.random_stream(300, 4000, seed=21, p_delete=0.2)
    e, o = make(lib, 300), Oracle(300)
    e.apply(ops)
    o.apply(ops)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    check_state(e, o, ops, np.random.default_rng(5))


def test_sim_queries_fresh_empty_graph(lib):
    e, o = make(lib, 50), Oracle(50)
    check_state(e, o, np.empty((0, 3), np.uint32), np.random.default_rng(6), m=2000)
    assert np.all(e.lookup_edges(np.arange(50), np.arange(50)) == NO_EDGE)
    rows, dests, vals = e.gather_neighbourhoods(np.arange(60))
    assert np.all(rows == 0) and len(dests) == 0 and len(vals) == 0


def test_sim_query_edge_cases(lib, streams):
    ops = streams.random_stream(100, 1500, seed=7, p_delete=0.1)
    e, o = make(lib, 100), Oracle(100)
    e.apply(ops)
    o.apply(ops)
    L = e.L
    # n = 0 lookups, k = 0 gathers
    assert len(e.lookup_edges([], [])) == 0
    assert L.ppcsr_lookup_edges(e.h, None, None, 0, None) == 0
    rows, dests, vals = e.gather_neighbourhoods([])
    assert list(rows) == [0] and len(dests) == 0 and len(vals) == 0
    tot = ctypes.c_uint64(7)
    assert L.ppcsr_gather_neighbourhoods(e.h, None, 0, None, None, None, 0, ctypes.byref(tot)) == 0 and tot.value == 0
    # repeated and out-of-range vertices
    verts = np.array([3, 3, 100, 5000, 0xFFFFFFFF, 3, 99], np.uint32)
    rows, dests, vals = e.gather_neighbourhoods(verts)
    for i, v in enumerate(verts):
        ref = o.get_neighbourhood(int(v)) if v < 100 else np.empty(0, np.int32)
        np.testing.assert_array_equal(dests[int(rows[i]):int(rows[i + 1])], ref)
    # the size query and ERANGE (as ppcsr_scan_all): cap < total writes cap edges and reports the total
    assert len(dests) > 4
    q = np.ascontiguousarray(verts)
    r = np.zeros(len(q) + 1, np.uint64)
    assert L.ppcsr_gather_neighbourhoods(e.h, q.ctypes.data, len(q), r.ctypes.data, None, None, 0, ctypes.byref(tot)) == 0
    assert tot.value == len(dests)
    np.testing.assert_array_equal(r, rows)
    d = np.full(len(dests), -7, np.int32)
    v = np.zeros(len(dests), np.uint32)
    cap = len(dests) - 3
    assert L.ppcsr_gather_neighbourhoods(e.h, q.ctypes.data, len(q), r.ctypes.data, d.ctypes.data, v.ctypes.data, cap, ctypes.byref(tot)) == 6
    assert tot.value == len(dests)
    np.testing.assert_array_equal(d[:cap], dests[:cap])
    np.testing.assert_array_equal(v[:cap], vals[:cap])
    assert np.all(d[cap:] == -7)
    # lookups of src >= n report no edge (the single call reports EINVAL)
    assert e.lookup_edges([100, 1 << 31], [0, 0]).tolist() == [NO_EDGE, NO_EDGE]


def test_sim_pppcsr_queries_match_partitions(lib, streams):
    """PPPCSR: routed by owner, answered per partition, returned in the caller's order"""
    pkg = load_pkg()
    n, P = 400, 4
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P, lib=lib)
    ops = streams.random_stream(n, 3000, seed=9, p_delete=0.2)
    pp.apply(ops)
    rng = np.random.default_rng(10)
    q = np.concatenate([ops[:, :2], np.stack([rng.integers(0, n + 50, 500), rng.integers(0, n, 500)], 1)]).astype(np.uint32)
    q = q[rng.permutation(len(q))]
    vals = pp.lookup_edges(q[:, 0], q[:, 1])
    starts = [pp.partition_start(k) for k in range(P)]
    parts = [pp.partition(k) for k in range(P)]
    for j in range(len(q)):
        s, d = int(q[j, 0]), int(q[j, 1])
        k = pp.get_partiton(s)
        assert vals[j] == parts[k].lookup_edges([s - starts[k]], [d])[0]
        if s < n:
            assert (vals[j] != NO_EDGE) == pp.edge_exists(s, d)
    verts = np.concatenate([np.arange(n + 20), rng.integers(0, n, 200)]).astype(np.uint32)
    verts = verts[rng.permutation(len(verts))]
    rows, dests, gv = pp.gather_neighbourhoods(verts)
    for i, v in enumerate(verts):
        k = pp.get_partiton(int(v))
        _, rd, rv = parts[k].gather_neighbourhoods([int(v) - starts[k]])
        np.testing.assert_array_equal(dests[int(rows[i]):int(rows[i + 1])], rd)
        np.testing.assert_array_equal(gv[int(rows[i]):int(rows[i + 1])], rv)
        if v < n:
            np.testing.assert_array_equal(rd, pp.get_neighbourhood(int(v)))


def test_sim_gather_multi_tile_scans(lib, streams):
    """more rows and chunks than one scan tile (4096) holds: the tile sums are scanned by a second level, the chunk -> row map
    by a multi-tile max-scan; with a hub whose range is many chunks long"""
    n = 3000
    hub = np.stack([np.full(2500, 5, np.uint32), np.arange(2500, dtype=np.uint32) * 3 + 1, np.arange(2500, dtype=np.uint32) + 2], 1)
    ops = np.concatenate([streams.random_stream(n, 12000, seed=12), hub])
    e, o = make(lib, n), Oracle(n)
    e.apply(ops)
    o.apply(ops)
    same_state(e, o)
    items, nodes = e.state()
    rng = np.random.default_rng(13)
    verts = np.concatenate([np.tile(np.arange(n), 3), np.full(40, 5), rng.integers(0, n + 10, 500)]).astype(np.uint32)
    verts = verts[rng.permutation(len(verts))]
    rows, dests, vals = e.gather_neighbourhoods(verts)
    assert len(verts) > 8192
    for i, v in enumerate(verts):
        sl = live_slots(items, nodes, int(v))
        np.testing.assert_array_equal(dests[int(rows[i]):int(rows[i + 1])], sl[:, 1].astype(np.int32), err_msg=f"row {i} ({v})")
        np.testing.assert_array_equal(vals[int(rows[i]):int(rows[i + 1])], sl[:, 2])
