"""GPU: ppcsr_label_propagation / ppcsr_modularity and their pppcsr_ forms on MI355X, all partitions on one device: against the
models of tests/community_model.py (the sequential sweep on Python integers where the size allows, the numpy replica of the steps
everywhere) and its order-blind validator — at RMAT scale 14 under streams and a repartition, once at scale 18 on 8 partitions
and on one PCSR, at the grid-stride seams of the vertex launches and of the streaming pass, on the hub graph with a 64-slot
table, and over a few rounds of batch-then-check, warm-started beside a cold start.  Every test first asserts, from the model,
the floors that keep its input hard."""
import ctypes

import numpy as np
import pytest

from colouring_model import assert_hard
from community_model import (WAVE_LIST, assert_maximisers, colours, hardness, model_sweeps, modularity_ints, replica_sweeps, weighted_csr)
from consumers_model import partition_states
from helpers import load_pkg
from paths_model import global_edges_valued

pytestmark = pytest.mark.gpu
ORDERS = ("random", "degree", "id")
STREAM_GRID_SLOTS = 1 << 23  # slots one step of a streaming pass covers: its grid stops growing at 8192 workgroups of 1024 slots
VERTEX_GRID = 1 << 20        # vertices one step of a vertex launch covers: 4096 workgroups of 256 threads
LIST_GRID_WAVES = 1 << 16    # class vertices one step of a step kernel covers: 16384 workgroups of four waves


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()
    return p


def to_device(ops):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(ops, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def model(edges, n, order, seed, weighted, init=None, max_sweeps=0, python_loops=True):
    src, dst, val = edges
    rows, nbr, wt = weighted_csr(src, dst, val, n, weighted)
    _, classes = colours(src, dst, n, ORDERS.index(order), seed)
    r = replica_sweeps(rows, nbr, wt, classes, init, max_sweeps)
    if python_loops:  # the definition itself, beside the replica
        s = model_sweeps(rows, nbr, wt, classes, init, max_sweeps)
        np.testing.assert_array_equal(r["labels"], s["labels"])
        assert {k: v for k, v in r.items() if k != "labels"} == {k: v for k, v in s.items() if k != "labels"}
    return rows, nbr, wt, r, hardness(rows, classes, r)


def check_modularity(g, rows, nbr, wt, labels, weighted, label):
    words, _, q = modularity_ints(rows, nbr, wt, labels)
    got_q, got, ms = g.modularity(labels, weighted, with_ms=True)
    print(f"{label}: modularity {ms:.3f} ms, q {got_q:.6f}, words {got.tolist()}")
    assert [int(x) for x in got] == words, (label, got, words)
    assert abs(got_q - q) <= 1e-12, (label, got_q, float(q))  # (five roundings of values <= 1: under 1e-15)


def compare(g, edges, n, order, seed, weighted, label, init=None, max_sweeps=0, python_loops=True, **hard):
    """one call against the model — the floors on the input first: labels, sweeps, communities, counters [0] - [5], the
    validator on a converged answer, the modularity of the answer"""
    rows, nbr, wt, r, h = model(edges, n, order, seed, weighted, init, max_sweeps, python_loops)
    assert_hard(h, label, **hard)
    labels, ncom, sweeps, ms = g.label_propagation(order, seed, weighted, max_sweeps, init, with_ms=True)
    c = g.debug_community_counters()
    print(f"{label}: label propagation {ms:.3f} ms, counters {c.tolist()}, model {h}")
    np.testing.assert_array_equal(labels, r["labels"], err_msg=f"{label}: labels")
    assert (ncom, sweeps) == (h["communities"], h["sweeps"]) and ms >= 0.0, (label, ncom, sweeps, h)
    assert tuple(int(x) for x in c[:6]) == (h["sweeps"], h["classes"], r["changes"], r["last"], h["communities"], h["block_tier"]), (label, c, h)
    if r["last"] == 0:
        assert_maximisers(rows, nbr, wt, labels, label)
    check_modularity(g, rows, nbr, wt, labels, weighted, label)
    return labels, r, h


def check_model(pp, label, runs, seed=7, python_loops=True, **hard):
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    edges = global_edges_valued(states)
    out = {(order, weighted): compare(pp, edges, n, order, seed, weighted, f"{label} {order} weighted={weighted}", None, 0, python_loops, **hard)
           for order, weighted in runs}
    for (_, i0, n0), (_, i1, n1) in zip(states, partition_states(pp)):  # nothing written
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1), label
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return edges, out


def weigh(adds, modulus):
    """values in [1, modulus] that depend on the pair alone (a bulk build keeps one of equal duplicates)"""
    adds = adds.copy()
    adds[:, 2] = 1 + (adds[:, 0].astype(np.uint64) * 7 + adds[:, 1].astype(np.uint64) * 13) % modulus
    return adds


def test_community_model_rmat14(pkg, streams):
    """P = 8: an RMAT core, a mixed stream over stored and fresh pairs with destinations >= n, add_node and edges to and from the
    new vertex, a repartition to balanced_starts; the three orders and both flags.  Floors rounded down from the model
    (5 - 6 sweeps, 22 - 29 classes, 15 - 17 thousand label changes, about 1000 decisions where the own label was one of several
    maxima and 3000 - 5000 where the smallest of several was taken, 422 lists of 65 .. 512 entries and 15 longer ones, 7267
    isolated vertices)"""
    n, P = 1 << 14, 8
    hard = dict(sweeps=4, classes=16, changes=12_000, own_ties=500, min_ties=2000, wave_tier=256, block_tier=8, isolated=4096)
    s, d = streams.rmat_edges(14, 120_000, seed=51)
    core = weigh(streams.adds(s, d), 3)
    s2, d2 = streams.rmat_edges(14, 2_000, seed=52)
    mixed = streams.mixed_existing_stream(core, streams.adds(s2, d2 + np.uint32(7)), seed=53)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    pp.apply(core)
    pp.apply(mixed)
    check_model(pp, "rmat14", [(o, w) for o in ORDERS for w in (False, True)], **hard)
    pp.add_node()
    pp.apply(np.array([[n, 1, 5], [2, n, 9], [1, n, 1], [0, n, 1], [1, 2, 1]], np.uint32))
    pp.add_node()  # (isolated unless the stream named it)
    _, out = check_model(pp, "rmat14 add_node", [("id", True)], **hard)
    assert out["id", True][0][n + 1] == n + 1
    pp.repartition(pp.balanced_starts())
    check_model(pp, "rmat14 repartitioned", [("degree", False), ("random", True)], **hard)
    pp.close()


def test_community_model_rmat18(pkg, streams):
    """once at scale 18, bulk-built from a device tensor on 8 partitions and on one PCSR, against the numpy replica: the lists
    of at most 64 entries of class 0 — one launch's list — beyond the list grid's 65536 waves, lists beyond the wave tier,
    several sweeps.  The floors are rounded down from the model (random unweighted / degree weighted: 5 / 6 sweeps, 69 / 47
    classes, 79442 / 71197 such vertices in class 0, 172 lists beyond 512 entries, the longest 9192)"""
    n = 1 << 18
    s, d = streams.rmat_edges(18, 2_000_000, seed=31)
    adds = weigh(streams.adds(s, d), 4)
    t = to_device(adds)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    pp.bulk_build_device(t.data_ptr(), len(adds))
    one = pkg.PCSR(n)
    one.bulk_build(adds)
    del t
    key, at = np.unique(adds[:, 0].astype(np.int64) * n + adds[:, 1].astype(np.int64), return_index=True)  # (the distinct pairs)
    edges = (key // n, key % n, adds[at, 2].astype(np.int64))
    for order, weighted in (("random", False), ("degree", True)):
        labels, r, h = compare(pp, edges, n, order, 3, weighted, f"rmat18 {order}", python_loops=False, class0_lane_tier=LIST_GRID_WAVES + 1,
                               maxdeg=WAVE_LIST + 1, block_tier=128, sweeps=3, classes=40)
        got, ncom, sweeps = one.label_propagation(order, 3, weighted)
        np.testing.assert_array_equal(got, labels)
        assert (ncom, sweeps) == (h["communities"], h["sweeps"])
        assert [int(x) for x in one.debug_community_counters()[:6]] == [int(x) for x in pp.debug_community_counters()[:6]]
    pp.close()
    one.close()


def test_community_vertex_grid_stride(pkg):
    """n = 2^20 + 777 with a sparse edge set (a random permutation's path broken every 16 vertices, and a few chords): the
    vertex launches stride, and the tail past 2^20 is part of the graph — its labels move and are checked.  (The model: 3 - 4
    sweeps, 5 classes, the widest of 455 thousand vertices, 710 thousand changes; 592 / 715 tail vertices end with another label
    and 447 / 124 vertices with a label from the tail)"""
    n = VERTEX_GRID + 777
    rng = np.random.default_rng(4)
    perm = rng.permutation(n).astype(np.int64)
    a, b = perm[:-1], perm[1:]
    keep = np.arange(n - 1) % 16 != 15
    ca, cb = rng.integers(0, n, 200_000), rng.integers(0, n, 200_000)
    key = np.unique(np.minimum(np.concatenate([a[keep], ca]), np.concatenate([b[keep], cb])) * n
                    + np.maximum(np.concatenate([a[keep], ca]), np.concatenate([b[keep], cb])))
    key = key[key // n != key % n]
    adds = np.stack([key // n, key % n, 1 + key % 3], axis=1).astype(np.uint32)
    g = pkg.PCSR(n)
    g.bulk_build(adds[rng.permutation(len(adds))])
    edges = (adds[:, 0].astype(np.int64), adds[:, 1].astype(np.int64), adds[:, 2].astype(np.int64))
    for order, weighted in (("random", True), ("id", False)):
        labels, r, h = compare(g, edges, n, order, 1, weighted, f"vertex stride {order}", python_loops=False, sweeps=3, classes=3,
                               widest_class=VERTEX_GRID // 4, changes=VERTEX_GRID // 2)
        tail = np.arange(VERTEX_GRID, n)
        assert np.count_nonzero(labels[tail] != tail) >= 500 and np.count_nonzero(labels >= VERTEX_GRID) >= 100
    g.close()


def test_modularity_pass_grid_stride(pkg):
    """modularity on arrays of more than 2^23 slots: the streaming pass's grid has stopped growing and every wave loops.
    n = 2^19, 14 pairs per vertex inside blocks of 64 consecutive ids; labels by block, by a coarse random map, and all one"""
    n, B = 1 << 19, 64
    rng = np.random.default_rng(9)
    v = np.repeat(np.arange(n, dtype=np.int64), 14)
    w = v - v % B + rng.integers(0, B, len(v))
    key = np.unique(v * n + w)  # (a bulk build takes distinct pairs)
    adds = np.stack([key // n, key % n, 1 + key % 1000], axis=1).astype(np.uint32)
    g = pkg.PCSR(n)
    g.bulk_build(adds[rng.permutation(len(adds))])
    slots = g.geometry()[0]
    assert slots > STREAM_GRID_SLOTS, slots
    edges = (adds[:, 0].astype(np.int64), adds[:, 1].astype(np.int64), adds[:, 2].astype(np.int64))
    assert (edges[0] > edges[1]).any() and (edges[0] == edges[1]).any()
    for weighted in (False, True):
        rows, nbr, wt = weighted_csr(*edges, n, weighted)
        for name, labels in (("blocks", np.arange(n) // B * B), ("random", rng.integers(0, 1000, n)), ("one", np.full(n, n - 1))):
            check_modularity(g, rows, nbr, wt, labels.astype(np.uint32), weighted, f"pass stride {name} weighted={weighted}")
    g.close()


def hub_graph(n, hub, rng):
    others = rng.permutation(np.setdiff1d(np.arange(n), [hub]))
    kq = others[5000:5100]
    i, j = np.triu_indices(100, 1)
    pairs = np.concatenate([np.stack([np.full(5060, hub), others[:5060]], axis=1), np.stack([kq[i], kq[j]], axis=1)])
    return np.stack([pairs.min(axis=1), pairs.max(axis=1), 1 + pairs.max(axis=1) % 4], axis=1).astype(np.uint32)


@pytest.mark.parametrize("hub", [0, 5999])
def test_community_small_table_on_the_hub_graph(pkg, hub):
    """a hub with 5060 neighbours, first and last in the id order: with lp_table_slots = 64 the workgroup's table overflows and
    the labels go through hash passes — counter [6] — and the answer equals the default table's"""
    n = 6000
    rng = np.random.default_rng(5)
    ops = hub_graph(n, hub, rng)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=2)
    pp.apply(ops[rng.permutation(len(ops))])
    edges = global_edges_valued(partition_states(pp))
    runs = (("id", 0, False), ("random", 6, True))  # (under `random` about half of the leaves move before the hub)
    default = {}
    for order, seed, weighted in runs:
        default[order], _, _ = compare(pp, edges, n, order, seed, weighted, f"hub {hub} {order}", python_loops=False, block_tier=1, maxdeg=5060)
    pp.partition(0).set_option("lp_table_slots", 64)
    for order, seed, weighted in runs:
        small, _, _ = compare(pp, edges, n, order, seed, weighted, f"hub {hub} {order}, 64 slots", python_loops=False)
        np.testing.assert_array_equal(small, default[order])
        if order == "random" or hub == 0:
            assert pp.debug_community_counters()[6] >= 1
    pp.close()


def test_community_follow_batches(pkg, streams):
    """3 rounds of: apply a batch of adds, deletes, a self-loop and a destination >= n, then a warm start from the previous
    labels beside a cold start, both against the model (cold: 6 sweeps and 17 - 22 thousand changes; warm: 4 sweeps and 2.7 - 6
    thousand)"""
    n, P = 1 << 14, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges(14, 60_000, seed=61)
    pp.apply(weigh(streams.adds(s, d), 3))
    previous = {o: pp.label_propagation(o, 2, True)[0] for o in ORDERS}
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 20_000, seed=62 + r)
        batch = np.concatenate([weigh(streams.adds(s2, d2), 3), streams.random_stream(n, 10_000, seed=80 + r, p_delete=0.5),
                                np.array([[r, r, 1], [r, n + r, 1]], np.uint32)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        edges = global_edges_valued(partition_states(pp))
        order = ORDERS[r]
        _, cold, _ = compare(pp, edges, n, order, 2, True, f"round {r} cold", sweeps=3, classes=16, changes=12_000)
        warm, rw, _ = compare(pp, edges, n, order, 2, True, f"round {r} warm", init=previous[order], sweeps=3, changes=2000)
        assert rw["changes"] < cold["changes"]
        previous[order] = warm
    pp.close()


def test_community_status_codes(pkg, streams):
    """argument errors with EINVAL; partitions on two devices refused with EUNSUPPORTED; the sequential regime answered"""
    n = 1 << 12
    s, d = streams.rmat_edges(12, 60_000, seed=41)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4)
    pp.apply(weigh(streams.adds(s, d), 5))
    L = pp.L
    labels, words = np.full(n, 77, np.uint32), np.full(4, 77, np.uint64)
    ncom, sweeps, q = ctypes.c_uint64(77), ctypes.c_uint32(77), ctypes.c_double(77.0)
    e = pp.partition(2)
    for lp, mod, h, m in ((L.pppcsr_label_propagation, L.pppcsr_modularity, pp.h, n), (L.ppcsr_label_propagation, L.ppcsr_modularity, e.h, e.get_n())):
        good, bad = np.zeros(m, np.uint32), np.full(m, m, np.uint32)
        assert lp(h, 0, 1, 0, 0, None, None, None, None, None) == 1 and mod(h, good.ctypes.data, 0, None, None, None) == 1
        assert lp(None, 0, 1, 0, 0, None, labels.ctypes.data, None, None, None) == 1 and mod(None, good.ctypes.data, 0, words.ctypes.data, None, None) == 1
        assert lp(h, 3, 1, 0, 0, None, labels.ctypes.data, ctypes.byref(ncom), ctypes.byref(sweeps), None) == 1
        assert lp(h, 0, 1, 2, 0, None, labels.ctypes.data, ctypes.byref(ncom), ctypes.byref(sweeps), None) == 1
        assert lp(h, 0, 1, 0, 0, bad.ctypes.data, labels.ctypes.data, ctypes.byref(ncom), ctypes.byref(sweeps), None) == 1
        assert mod(h, good.ctypes.data, 6, words.ctypes.data, ctypes.byref(q), None) == 1
        assert mod(h, bad.ctypes.data, 0, words.ctypes.data, ctypes.byref(q), None) == 1 and mod(h, None, 0, words.ctypes.data, None, None) == 1
    assert np.all(labels == 77) and np.all(words == 77) and (ncom.value, sweeps.value, q.value) == (77, 77, 77.0)  # nothing written
    assert L.ppcsr_set_option(e.h, b"lp_table_slots", 96) == 1 and L.ppcsr_set_option(e.h, b"lp_table_slots", 4096) == 0
    edges = global_edges_valued(partition_states(pp))
    rows, nbr, wt, want, h = model(edges, n, "degree", 1, True)
    assert h["sweeps"] >= 3 and h["communities"] >= 2
    assert L.pppcsr_label_propagation(pp.h, 1, 1, 1, 0, None, None, ctypes.byref(ncom), ctypes.byref(sweeps), None) == 0
    assert (ncom.value, sweeps.value) == (h["communities"], h["sweeps"])
    assert L.pppcsr_label_propagation(pp.h, 1, 1, 1, 0, None, labels.ctypes.data, None, None, None) == 0
    np.testing.assert_array_equal(labels, want["labels"])
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    tri = np.empty(n, np.uint64)
    assert L.pppcsr_triangles(pp.h, tri.ctypes.data, None, None) == 4  # (the regime triangles refuses)
    np.testing.assert_array_equal(pp.label_propagation("degree", 1, True)[0], want["labels"])
    check_modularity(pp, rows, nbr, wt, want["labels"], True, "sequential regime")
    assert len(e.label_propagation()[0]) == e.get_n()
    e.set_option("search_narrow", 1)
    if L.ppcsr_device_count() >= 2:
        two = pkg.PPPCSR(n, numDomain=2, partitionsPerDomain=1, devices=[0, 1])
        assert L.pppcsr_label_propagation(two.h, 0, 1, 0, 0, None, labels.ctypes.data, None, None, None) == 4
        assert "more than one device" in L.ppcsr_last_error().decode()
        assert L.pppcsr_modularity(two.h, labels.ctypes.data, 0, words.ctypes.data, None, None) == 4
        assert "more than one device" in L.ppcsr_last_error().decode()
    pp.close()
