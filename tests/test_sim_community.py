"""CPU: ppcsr_label_propagation / ppcsr_modularity and their pppcsr_ forms on the fiber SIMT emulator (tests/hostsim), which
compiles the engine's own kernel and host source.  Labels, sweeps, communities and every graph-determined counter are checked
exactly against tests/community_model.py (a sequential sweep on Python integers and a numpy replica of the steps), built from the
exported partition states, against the order-blind validator and against closed forms."""
import ctypes

import numpy as np
import pytest

from colouring_model import assert_hard
from community_model import (LANE_LIST, WAVE_LIST, assert_maximisers, colours, hardness, model_sweeps, modularity_ints, replica_sweeps,
                             weighted_csr)
from consumers_model import last_slot_free, partition_states
from helpers import load_pkg
from paths_model import global_edges_valued
from test_sim_colouring import clique, hub_graph, star, upper
from test_sim_engine import SIM_SO, build_sim
from test_sim_kcore import alloc_failures
from test_sim_pppcsr_consumers import make, mixed_stream, tune

EINVAL, ENOMEM, EHIP, EUNSUPPORTED = 1, 2, 3, 4
ORDERS = ("random", "degree", "id")
TOP = 2 ** 32 - 2  # the largest value a live edge stores (2^32 - 1 marks a sentinel)


@pytest.fixture(scope="module")
def lib():
    build_sim()
    L = load_pkg().load_library(SIM_SO)
    L.ppcsr_sim_fail_alloc_after.argtypes = [ctypes.c_int]
    return L


def model(edges, n, order, seed, weighted, init=None, max_sweeps=0, python_loops=True):
    """everything the device must reproduce for one call"""
    src, dst, val = edges
    rows, nbr, wt = weighted_csr(src, dst, val, n, weighted)
    _, classes = colours(src, dst, n, ORDERS.index(order), seed)
    r = replica_sweeps(rows, nbr, wt, classes, init, max_sweeps)
    if python_loops:  # the definition itself, beside the replica
        s = model_sweeps(rows, nbr, wt, classes, init, max_sweeps)
        np.testing.assert_array_equal(r["labels"], s["labels"])
        assert {k: v for k, v in r.items() if k != "labels"} == {k: v for k, v in s.items() if k != "labels"}
    return rows, nbr, wt, r, hardness(rows, classes, r)


def compare(pp, edges, n, order, seed, weighted, label, init=None, max_sweeps=0, python_loops=True):
    """one call against the model: labels, sweeps, communities, counters [0] - [5]; converged answers pass the validator; the
    modularity of the answer: four exact words and q"""
    rows, nbr, wt, r, h = model(edges, n, order, seed, weighted, init, max_sweeps, python_loops)
    labels, ncom, sweeps, ms = pp.label_propagation(order, seed, weighted, max_sweeps, init, with_ms=True)
    np.testing.assert_array_equal(labels, r["labels"], err_msg=f"{label}: labels")
    assert (ncom, sweeps) == (h["communities"], h["sweeps"]) and ms >= 0.0, (label, ncom, sweeps, h)
    c = pp.debug_community_counters()
    assert tuple(int(x) for x in c[:6]) == (h["sweeps"], h["classes"], r["changes"], r["last"], h["communities"], h["block_tier"]), (label, c, h)
    assert c[7] >= c[0]
    if r["last"] == 0:
        assert_maximisers(rows, nbr, wt, labels, label)
    check_modularity(pp, rows, nbr, wt, labels, weighted, label)
    return labels, r, h


def check_modularity(pp, rows, nbr, wt, labels, weighted, label):
    words, _, q = modularity_ints(rows, nbr, wt, labels)
    got_q, got = pp.modularity(labels, weighted)
    assert [int(x) for x in got] == words, (label, got, words)
    # (the double expression makes five roundings of values <= 1: under 1e-15)
    assert abs(got_q - float(q)) <= 1e-12 and abs(got_q - q) <= 1e-12, (label, got_q, q)


def check(pp, label, orders=ORDERS, seed=7, flags=(False, True), **hard):
    """every order and both flags against the model, the floors on the input; nothing written (states and stats)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    edges = global_edges_valued(states)
    out = {}
    for order in orders:
        for weighted in flags:
            out[order, weighted] = compare(pp, edges, n, order, seed, weighted, f"{label} {order} weighted={weighted}")
            assert_hard(out[order, weighted][2], f"{label} {order}", **hard)
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return edges, out


def valued(pairs, values):
    """rows (min, max, value) of undirected pairs"""
    ops = upper(pairs)
    ops[:, 2] = np.asarray(values, np.uint64).astype(np.uint32)
    return ops


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_community_model(lib, streams, P):
    """a bulk-built folded RMAT core under a mixed stream (deletes, duplicate adds, destinations >= n), add_node twice and edges
    to and from the new vertices, a repartition to balanced_starts.  P = 3 runs with every wv::uni / wv::bcast verified"""
    n = 1200
    hard = dict(sweeps=3, classes=6, changes=800, communities=2, own_ties=5, min_ties=5, wave_tier=1, isolated=1)
    lib.ppcsr_sim_check_uniform(1 if P == 3 else 0)
    try:
        pp = make(lib, n, P)
        s, d = streams.rmat_edges_folded(n, 11, 8000, seed=41)
        adds = np.concatenate([streams.adds(s, d), np.array([[5, 5, 1]], np.uint32)])
        adds[:, 2] = 1 + np.random.default_rng(P).integers(0, 3, len(adds))  # (small weights: ties stay frequent)
        pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
        ops = mixed_stream(streams, n, seed=40 + P)
        pp.apply(ops[: len(ops) // 2])
        pp.apply(ops[len(ops) // 2:])
        check(pp, f"P={P}", **hard)
        pp.add_node()
        pp.add_node()
        pp.apply(np.array([[n, 3, 2], [7, n, 3], [3, n, 1], [9, n, 1], [n, n + 1, 1], [n + 5, 1, 1], [n + 1, n + 9, 1]], np.uint32))
        check(pp, f"P={P} add_node", orders=("random",), **hard)
        pp.repartition(pp.balanced_starts())
        tune(pp)
        check(pp, f"P={P} repartitioned", orders=("degree",), **hard)
        pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


@pytest.mark.parametrize("P", [1, 4])
def test_sim_community_closed_forms(lib, P):
    """disjoint cliques end with one label each — the smallest id of the clique other than its first vertex in the order — and
    isolated vertices keep theirs; K_{20,20} and the path of 600 vertices, where a fully synchronous update flips for ever,
    converge with counter [3] == 0"""
    n = 400
    rng = np.random.default_rng(3 + P)
    perm = rng.permutation(n)
    cliques = [perm[:30], perm[30:37], perm[37:39]]
    lone = perm[39:]
    ops = upper(np.concatenate([clique(c) for c in cliques]))
    pp = make(lib, n, P)
    pp.apply(ops[rng.permutation(len(ops))])
    edges = global_edges_valued(partition_states(pp))
    for order in ORDERS:
        labels, r, h = compare(pp, edges, n, order, 9, False, f"cliques {order}")
        colour, _ = pp.colouring(order, 9)
        for c in cliques:
            first = c[np.argmin(colour[c])]  # (colour 0 of the clique: its first vertex in the order)
            assert np.all(labels[c] == np.setdiff1d(c, [first]).min()), (order, c, labels[c])
        np.testing.assert_array_equal(labels[lone], lone)
        assert h["communities"] == len(cliques) + len(lone) and pp.debug_community_counters()[3] == 0
    pp.close()
    m, L = 20, 600
    n = 2 * m + L
    ai, bj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    ops = upper(np.concatenate([np.stack([ai.ravel(), bj.ravel() + m], axis=1), np.stack([np.arange(L - 1), np.arange(1, L)], axis=1) + 2 * m]))
    pp = make(lib, n, P)
    pp.apply(ops[rng.permutation(len(ops))])
    edges = global_edges_valued(partition_states(pp))
    for order in ORDERS:
        labels, r, h = compare(pp, edges, n, order, 2, False, f"bipartite {order}")
        assert r["last"] == 0 and pp.debug_community_counters()[3] == 0
        assert len(np.unique(labels[:2 * m])) == 1  # (K_{20,20} agrees on one label)
    pp.close()


def test_sim_community_crafted_starts(lib):
    """the two tie rules, a 64-bit score, max_sweeps, and the warm start, on a star whose centre 0 sees crafted labels"""
    n = 40
    leaves = np.arange(1, 10)
    pp = make(lib, n, 2)
    # leaves 1-3 weigh TOP each, leaf 4 weighs TOP too, leaves 5-9 weigh 1; 20 - 21 is an edge apart
    pp.apply(valued(np.concatenate([star(0, leaves), [[20, 21]]]), [TOP, TOP, TOP, TOP, 1, 1, 1, 1, 1, 5]))
    edges = global_edges_valued(partition_states(pp))

    def centre(init, weighted, max_sweeps=1):
        start = np.arange(n, dtype=np.uint32)
        start[:len(init)] = init
        labels, r, _ = compare(pp, edges, n, "id", 0, weighted, f"crafted {init}", init=start, max_sweeps=max_sweeps)
        return int(labels[0]), r
    # (under `id` the centre is class 0 and moves first, against the crafted labels)
    assert centre([30, 7, 7, 30, 30, 30, 5, 9, 9, 9], False)[0] == 30  # the own label 30 ties with 9 at 3: kept, although 9 < 30
    assert centre([31, 7, 7, 30, 30, 30, 5, 9, 9, 9], False)[0] == 9   # 9 and 30 score 3 and neither is the own label: the smallest
    assert centre([31, 7, 7, 30, 30, 5, 5, 9, 9, 9], False)[0] == 9    # 9 scores 3 alone
    # weighted: three edges of weight TOP carry label 7 — 3 (2^32 - 2) > 2^33 — against label 30 on ONE edge of weight TOP; in
    # 32-bit arithmetic 3 TOP wraps to 2^32 - 6 < TOP and label 30 would win
    crafted = [31, 7, 7, 7, 30, 11, 12, 13, 14, 15]
    assert centre(crafted, True)[0] == 7 and 3 * TOP > 2 ** 33 and TOP > (3 * TOP) % 2 ** 32
    assert centre([30] + crafted[1:], True)[0] == 7  # (nor does the own label's TOP reach it)
    assert centre(crafted, False)[0] == 7
    pp.close()


def test_sim_community_sweep_limits_and_warm_start(lib, streams):
    """max_sweeps = 1 and 2 stop early with counter [3] > 0; a warm start from a converged answer runs exactly one sweep; after a
    batch the warm start and the cold start both equal the model"""
    n = 900
    pp = make(lib, n, 3)
    s, d = streams.rmat_edges_folded(n, 10, 6000, seed=12)
    adds = streams.adds(s, d)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    edges = global_edges_valued(partition_states(pp))
    for k in (1, 2):
        _, r, h = compare(pp, edges, n, "random", 3, False, f"max_sweeps={k}", max_sweeps=k)
        assert r["sweeps"] == k and r["last"] > 0 and pp.debug_community_counters()[3] == r["last"]
    full, r, h = compare(pp, edges, n, "random", 3, False, "converged")
    assert h["sweeps"] >= 3 and r["last"] == 0
    warm, r, _ = compare(pp, edges, n, "random", 3, False, "warm", init=full)
    assert r["sweeps"] == 1 and r["changes"] == 0
    np.testing.assert_array_equal(warm, full)
    pp.apply(mixed_stream(streams, n, seed=2))
    edges = global_edges_valued(partition_states(pp))
    for weighted in (False, True):
        _, rw, _ = compare(pp, edges, n, "random", 3, weighted, "warm after a batch", init=full)
        _, rc, _ = compare(pp, edges, n, "random", 3, weighted, "cold after a batch")
        assert rw["changes"] >= 1 and rw["changes"] < rc["changes"]  # (the previous answer is most of the way there)
    pp.close()


@pytest.mark.parametrize("hubs_first", [False, True])
def test_sim_community_list_length_seams(lib, hubs_first):
    """hubs with exactly 64 / 65 neighbours (registers / the wave's table) and 512 / 513 (the wave's table / the workgroup's),
    first or last in the id order, their leaves in groups that carry crafted labels of known scores"""
    sizes = {"h64": LANE_LIST, "h65": LANE_LIST + 1, "h512": WAVE_LIST, "h513": WAVE_LIST + 1}
    n = 1400
    hub = {name: (i if hubs_first else n - 4 + i) for i, name in enumerate(sizes)}
    pairs, at = [], 10
    init = np.arange(n, dtype=np.uint32)
    want = {}
    for name, k in sizes.items():
        leaves = np.arange(at, at + k)
        at += k
        pairs.append(star(hub[name], leaves))
        # a third of the leaves carries the label of the first leaf, a third less one that of the last: the larger group wins
        third = k // 3
        init[leaves[:third]] = leaves[0]
        init[leaves[k - third + 1:]] = leaves[-1]
        want[name] = leaves[0]
    pp = make(lib, n, 2)
    ops = upper(np.concatenate(pairs))
    ops[:, 2] = 1 + (ops[:, 1] % 3)
    ops = ops[np.random.default_rng(8).permutation(len(ops))]
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    edges = global_edges_valued(partition_states(pp))
    for weighted in (False, True):
        _, _, h = compare(pp, edges, n, "id", 0, weighted, f"seams first={hubs_first}")
        assert (h["wave_tier"], h["block_tier"]) == (2, 1)
        labels, r, _ = compare(pp, edges, n, "id", 0, weighted, f"seams crafted first={hubs_first}", init=init, max_sweeps=1)
        if hubs_first and not weighted:  # (the hubs move first, against the crafted labels)
            assert [int(labels[hub[k]]) for k in sizes] == [int(want[k]) for k in sizes]
        compare(pp, edges, n, "random", 12, weighted, f"seams random first={hubs_first}")
    pp.close()


@pytest.mark.parametrize("P,hub", [(1, 0), (3, 5999)])
def test_sim_community_hub_and_small_table(lib, P, hub):
    """a hub with 5060 neighbours, first and last in the id order.  In the first sweep it sees as many labels as it has
    neighbours: with lp_table_slots = 64 the workgroup's table overflows, the labels go through hash passes (counter [6] >= 1)
    and the result equals the default table's"""
    n = 6000
    rng = np.random.default_rng(P)
    leaves, kq, ops = hub_graph(n, hub, rng)
    ops[:, 2] = 1 + (ops[:, 1] % 4)
    runs = (("id", 0), ("random", 6))  # (under `random` about half of the leaves move before the hub and half after)
    pp = make(lib, n, P)
    ops = ops[rng.permutation(len(ops))]
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    edges = global_edges_valued(partition_states(pp))
    default = {}
    for order, seed in runs:
        for weighted in (False, True):
            default[order, weighted], _, h = compare(pp, edges, n, order, seed, weighted, f"hub P={P} {order}", python_loops=False)
            assert h["block_tier"] == 1 and h["maxdeg"] == 5060
        if order == "id" and hub == 0:  # (the first vertex sees 5060 labels: more than 3/4 of 4096 slots)
            assert pp.debug_community_counters()[6] >= 1
    pp.partition(0).set_option("lp_table_slots", 64)
    for order, seed in runs:
        for weighted in (False, True):
            small, _, _ = compare(pp, edges, n, order, seed, weighted, f"hub P={P} {order}, 64 slots", python_loops=False)
            np.testing.assert_array_equal(small, default[order, weighted])
            if order == "random" or hub == 0:
                assert pp.debug_community_counters()[6] >= 1
    pp.close()


def test_sim_community_invariant(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and one graph before and after a repartition with an empty partition: equal results;
    P = 1 equals the partition's own engine call"""
    n = 1000
    s, d = streams.rmat_edges_folded(n, 10, 5000, seed=6)
    adds, ops = streams.adds(s, d), mixed_stream(streams, n, seed=5)
    results = []

    def both(x):
        out = []
        for o, weighted in (("random", False), ("degree", True), ("id", True)):
            labels, ncom, sweeps = x.label_propagation(o, 21, weighted)
            out.append((labels, ncom, sweeps, x.modularity(labels, weighted)[1].tolist()))
        return out
    for P in (1, 2, 4, 8):
        pp = make(lib, n, P)
        pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
        pp.apply(ops)
        assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
        results.append(both(pp))
        if P == 1:
            results.append(both(pp.partition(0)))
            check(pp, "invariant", orders=("random", "id"), seed=21, sweeps=3)
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
            tune(pp)
            results.append(both(pp))
        pp.close()
    for r in results[1:]:
        for x, y in zip(r, results[0]):
            np.testing.assert_array_equal(x[0], y[0])
            assert x[1:] == y[1:]


def test_sim_community_modularity(lib, streams):
    """the model's labels, the identity and the all-one labels, both flags: four exact words and q; heavy weights fill the high
    word of the sum of squares"""
    n = 800
    pp = make(lib, n, 3)
    s, d = streams.rmat_edges_folded(n, 10, 5000, seed=31)
    adds = streams.adds(s, d)
    adds[:, 2] = np.where(np.arange(len(adds)) % 3 == 0, TOP, 1 + np.arange(len(adds)) % 1000)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    pp.apply(np.array([[5, 5, 9], [9, 2, 3], [4, n + 2, 7]], np.uint32))  # a self-loop, a backward pair, a destination beyond n
    edges = global_edges_valued(partition_states(pp))
    for weighted in (False, True):
        rows, nbr, wt, r, h = model(edges, n, "random", 4, weighted, python_loops=False)
        for name, labels in (("model", r["labels"]), ("identity", np.arange(n, dtype=np.uint32)), ("one", np.ones(n, np.uint32))):
            check_modularity(pp, rows, nbr, wt, labels, weighted, f"{name} weighted={weighted}")
        words = modularity_ints(rows, nbr, wt, np.ones(n, np.uint32))[0]
        assert words[0] == words[1] and (words[3] > 0) == weighted
        q, _ = pp.modularity(np.ones(n, np.uint32), weighted)
        assert abs(q) <= 1e-12  # (one community: 1 - 1)
    # no edge at all: q = 0
    empty = make(lib, 10, 2)
    q, words = empty.modularity(np.arange(10, dtype=np.uint32))
    assert q == 0.0 and not words.any()
    labels, ncom, sweeps = empty.label_propagation()
    assert labels.tolist() == list(range(10)) and (ncom, sweeps) == (10, 1)
    assert [int(x) for x in empty.debug_community_counters()[:6]] == [1, 0, 0, 0, 10, 0]
    empty.close()
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_community_answers_in_the_sequential_regime(lib, streams, P):
    """narrow == 0 on one partition: neither call is refused (they intersect nothing) and both equal the model"""
    n = 500
    pp = make(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 9, 6000, seed=23)
    adds = streams.adds(s, d)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    e = pp.partition(P - 1)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    tri = np.empty(n, np.uint64)
    assert pp.L.pppcsr_triangles(pp.h, tri.ctypes.data, None, None) == EUNSUPPORTED  # (the regime is the one triangles refuses)
    check(pp, f"sequential P={P}", orders=("random",), sweeps=3)
    assert len(e.label_propagation()[0]) == e.get_n()
    assert e.stats()["narrow"] == 0
    pp.close()


def test_sim_community_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    L, h = pp.L, pp.h
    e = pp.partition(0)
    pp.apply(streams.random_stream(n, 1500, seed=1))
    edges = global_edges_valued(partition_states(pp))
    _, _, _, want, hh = model(edges, n, "random", 5, False)
    labels = np.full(n, 77, np.uint32)
    ncom, sweeps, ms, q = ctypes.c_uint64(77), ctypes.c_uint32(77), ctypes.c_double(), ctypes.c_double(77.0)
    words = np.full(4, 77, np.uint64)
    for lp, mod, hd, m in ((L.pppcsr_label_propagation, L.pppcsr_modularity, h, n), (L.ppcsr_label_propagation, L.ppcsr_modularity, e.h, e.get_n())):
        good = np.zeros(m, np.uint32)
        assert lp(hd, 0, 5, 0, 0, None, None, None, None, None) == EINVAL
        assert lp(None, 0, 5, 0, 0, None, labels.ctypes.data, None, None, None) == EINVAL
        assert mod(None, good.ctypes.data, 0, words.ctypes.data, None, None) == EINVAL
        assert mod(hd, None, 0, words.ctypes.data, None, None) == EINVAL
        assert mod(hd, good.ctypes.data, 0, None, None, None) == EINVAL
        for order, flags in ((3, 0), (0xFFFFFFFF, 0), (0, 2), (0, 3), (1, 0x80000000)):
            assert lp(hd, order, 5, flags, 0, None, labels.ctypes.data, ctypes.byref(ncom), ctypes.byref(sweeps), None) == EINVAL
        for flags in (2, 3, 0x80000000):
            assert mod(hd, good.ctypes.data, flags, words.ctypes.data, ctypes.byref(q), None) == EINVAL
        for bad in (m, m + 1, 0xFFFFFFFF):  # an entry that is no vertex id, in init and in labels
            start = np.zeros(m, np.uint32)
            start[m // 2] = bad
            assert lp(hd, 0, 5, 0, 0, start.ctypes.data, labels.ctypes.data, ctypes.byref(ncom), ctypes.byref(sweeps), None) == EINVAL
            assert mod(hd, start.ctypes.data, 0, words.ctypes.data, ctypes.byref(q), None) == EINVAL
        assert np.all(labels == 77) and np.all(words == 77) and (ncom.value, sweeps.value, q.value) == (77, 77, 77.0)  # nothing written
        # every output may be NULL alone
        assert lp(hd, 0, 5, 0, 0, None, None, ctypes.byref(ncom), None, None) == 0 and 1 <= ncom.value <= m
        assert lp(hd, 0, 5, 0, 0, None, None, None, ctypes.byref(sweeps), ctypes.byref(ms)) == 0 and sweeps.value >= 1 and ms.value >= 0.0
        assert lp(hd, 0, 5, 0, 0, None, labels.ctypes.data, None, None, None) == 0
        assert len(np.unique(labels[:m])) == ncom.value and np.all(labels[m:] == 77)
        assert mod(hd, labels.ctypes.data, 0, None, ctypes.byref(q), None) == 0 and -0.5 <= q.value <= 1.0
        assert mod(hd, labels.ctypes.data, 0, words.ctypes.data, None, ctypes.byref(ms)) == 0 and words[1] <= words[0]
        labels[:], words[:], ncom.value, sweeps.value, q.value = 77, 77, 77, 77, 77.0
    assert L.pppcsr_label_propagation(h, 0, 5, 0, 0, None, labels.ctypes.data, ctypes.byref(ncom), ctypes.byref(sweeps), None) == 0
    np.testing.assert_array_equal(labels, want["labels"])
    assert (ncom.value, sweeps.value) == (hh["communities"], hh["sweeps"])
    assert L.ppcsr_debug_community_counters(None, words.ctypes.data) == EINVAL and L.ppcsr_debug_community_counters(e.h, None) == EINVAL
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_label_propagation(loc.h, 0, 5, 0, 0, None, labels.ctypes.data, None, None, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_modularity(loc.h, labels.ctypes.data, 0, words.ctypes.data, None, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one — tests/test_gpu_community.py)
    # the option: powers of two in [64, 4096]
    for v in (64, 128, 1024, 4096):
        assert L.ppcsr_set_option(e.h, b"lp_table_slots", v) == 0, v
    for v in (0, 1, 32, 63, 65, 96, 4095, 4097, 8192, -64, 1 << 40):
        assert L.ppcsr_set_option(e.h, b"lp_table_slots", v) == EINVAL, v
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("what", ["unweighted", "weighted", "modularity"])
def test_sim_community_allocation_failures(lib, streams, what, P):
    """every device allocation of the call fails in turn: ENOMEM comes back, the state is unchanged, and the next call succeeds
    and equals the model"""
    def prepare(pp, states):
        n = pp.get_n()
        weighted = what != "unweighted"
        rows, nbr, wt, r, _ = model(global_edges_valued(states), n, "degree", 3, weighted)
        words = modularity_ints(rows, nbr, wt, r["labels"])[0]
        labels, out = np.empty(n, np.uint32), np.zeros(4, np.uint64)
        ncom, sweeps = ctypes.c_uint64(), ctypes.c_uint32()

        def verify(k):
            got, count, _ = pp.label_propagation("degree", 3, weighted)
            np.testing.assert_array_equal(got, r["labels"])
            assert count == len(np.unique(r["labels"]))
            assert pp.modularity(got, weighted)[1].tolist() == words
        if what == "modularity":
            return lambda k: pp.L.pppcsr_modularity(pp.h, r["labels"].ctypes.data, 1, out.ctypes.data, None, None), lambda k: ENOMEM, verify
        return (lambda k: pp.L.pppcsr_label_propagation(pp.h, 1, 3, int(weighted), 0, None, labels.ctypes.data, ctypes.byref(ncom),
                                                        ctypes.byref(sweeps), None), lambda k: ENOMEM, verify)
    # label propagation: the colouring's thirteen, the counters, (the weighted adjacency,) the buckets; modularity: the table,
    # labels, tot, partials, counters
    alloc_failures(lib, streams, P, prepare, {"unweighted": 15, "weighted": 16, "modularity": 5}[what])
