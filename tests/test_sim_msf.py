"""CPU: ppcsr_msf / pppcsr_msf on the fiber SIMT emulator (tests/hostsim), which compiles the engine's own kernel and host
source.  Edges, count, weight and labels are checked exactly against tests/msf_model.py (Kruskal on the distinct keys (w, lo, hi),
built from the exported partition states) and against closed forms; the counters of ppcsr_debug_msf_counters are checked against
the model's synchronous replica of the schedule.  The schedule fixes passes = 2 * rounds - 1: the last round, which finds no
cut edge, makes the first of its two passes only; and host reads = rounds + pointer-jump launches + 1."""
import ctypes

import numpy as np
import pytest

from consumers_model import last_slot_free, partition_states
from helpers import ERANGE, load_pkg
from msf_model import HARD, assert_hard, hardness, model_msf, model_rounds, ruler_path, zoo
from paths_model import global_edges_valued
from test_sim_engine import SIM_SO, build_sim
from test_sim_kcore import alloc_failures
from test_sim_paths import weigh
from test_sim_pppcsr_consumers import make, mixed_stream, tune

EINVAL, EHIP, EUNSUPPORTED = 1, 3, 4
BIG = 0xFFFFFFFE  # the largest value an edge can hold


@pytest.fixture(scope="module")
def lib():
    build_sim()
    L = load_pkg().load_library(SIM_SO)
    L.ppcsr_sim_fail_alloc_after.argtypes = [ctypes.c_int]
    return L


def check_counters(c, hooks, n, count, label):
    """the counters of the last call against the model's rounds (hooks per hooking round)"""
    assert int(c[0]) == len(hooks) + 1, (label, c, hooks)
    assert int(c[4]) == (hooks[0] if hooks else 0), (label, c, hooks)
    assert int(c[5]) == count == sum(hooks) and int(c[6]) == n - count, (label, c, count)
    assert int(c[0]) <= int(np.floor(np.log2(n))) + 1, (label, c)
    assert int(c[3]) <= int(np.ceil(np.log2(n))) + 1, (label, c)
    assert int(c[1]) == 2 * int(c[0]) - 1, (label, c)  # the last round makes its first pass only
    assert int(c[2]) >= len(hooks) and int(c[3]) <= int(c[2]), (label, c)
    assert int(c[7]) == int(c[0]) + int(c[2]) + 1 and c[7] >= c[0], (label, c)  # one read per round and per jump launch, one for the list's length


def check(pp, label, **hard):
    """edges, count, weight and labels against the model, labels against components(), the counters against the model's rounds;
    nothing written (states and stats); returns (edges, weight, labels, hardness)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst, val = global_edges_valued(states)
    want_e, want_w, want_l = model_msf(src, dst, val, n)
    h = hardness(src, dst, val, n, want_e)
    assert_hard(h, label, **hard)
    edges, weight, labels = pp.msf()
    np.testing.assert_array_equal(edges.astype(np.int64), want_e, err_msg=f"{label}: edges")
    assert weight == want_w and isinstance(weight, int), (label, weight, want_w)
    np.testing.assert_array_equal(labels, want_l, err_msg=f"{label}: labels")
    c = pp.debug_msf_counters()
    check_counters(c, h["hooks"], n, len(edges), label)
    np.testing.assert_array_equal(labels, pp.components(), err_msg=f"{label}: components")
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return edges, weight, labels, h


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_msf_model(lib, streams, P):
    """the zoo in two batches; a mixed stream with deletes and duplicate adds that overwrite values; add_node three times
    with edges to and from the new vertices (one left isolated); a repartition to balanced_starts: everything after each step.
    P = 3 runs with every wv::uni / wv::bcast verified"""
    n = 1200
    lib.ppcsr_sim_check_uniform(1 if P == 3 else 0)
    try:
        pp = make(lib, n, P)
        assert not pp.debug_msf_counters().any()  # all zeros before the first call
        assert not pp.partition(P - 1).debug_msf_counters().any()
        ops = zoo(streams, n, 11, 3000, seed=17)
        pp.apply(ops[: len(ops) // 2])
        pp.apply(ops[len(ops) // 2:])
        check(pp, f"P={P}", **HARD)
        pp.apply(weigh(streams, mixed_stream(streams, n, seed=40 + P), 4, seed=5 + P))
        check(pp, f"P={P} mixed", ties=1, opposite=1, reverse_only=1, beyond=1, isolated=1, rounds=3)  # (denser: one tree may be all)
        pp.add_node()
        pp.add_node()
        pp.add_node()
        pp.apply(np.array([[n, 3, 2], [3, n, 1], [n, n + 1, BIG], [n + 5, 1, 1], [n + 1, n + 9, 1]], np.uint32))
        edges, _, labels, _ = check(pp, f"P={P} add_node", beyond=1, isolated=1)
        rows = {(int(a), int(b)): int(w) for a, b, w in edges}
        # 3 <-> n: only the lighter direction can be a forest edge; n + 1 hangs on n unless an earlier destination >= n reached it
        assert rows.get((3, n), 1) == 1 and labels[n] == labels[3] == labels[n + 1] and rows.get((n, n + 1), BIG) == BIG
        pp.repartition(pp.balanced_starts())
        tune(pp)
        edges2, weight2, labels2, _ = check(pp, f"P={P} repartitioned")
        np.testing.assert_array_equal(edges2, edges)
        np.testing.assert_array_equal(labels2, labels)
        pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


def build(lib, n, P, rows, rng):
    """rows (src, dst, value) in a shuffled order on P partitions"""
    ops = np.asarray(rows, np.int64).astype(np.uint32)
    pp = make(lib, n, P)
    pp.apply(ops[rng.permutation(len(ops))])
    return pp


def rows_of(a, b, w):
    return np.stack([np.asarray(a, np.int64), np.asarray(b, np.int64), np.broadcast_to(np.asarray(w, np.int64), np.shape(a))], axis=1)


def expect(edges, weight, labels, rows, n, label):
    """the result is exactly the undirected `rows` (a forest), with their weight sum and the labels of their trees"""
    rows = np.asarray(rows, np.int64)
    want = np.stack([rows[:, :2].min(axis=1), rows[:, :2].max(axis=1), rows[:, 2]], axis=1)
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    np.testing.assert_array_equal(edges.astype(np.int64), want, err_msg=label)
    assert weight == sum(int(x) for x in want[:, 2].tolist()), label
    _, _, want_l = model_msf(rows[:, 0], rows[:, 1], rows[:, 2], n)
    np.testing.assert_array_equal(labels, want_l, err_msg=label)


@pytest.mark.parametrize("P", [1, 4])
def test_sim_msf_closed_forms(lib, P):
    """on permuted ids: the ruler path on 2^7 vertices (exactly 7 hooking rounds + the empty one, hooks 64, 32, ..., 1); an
    ascending-weight path of 600 (one hooking round, one chain 599 deep, at most 11 jump launches); a star with 500 leaves of
    the largest value, stored outward and inward (weight beyond 2^32); K_40 with all weights 1 (the star of its smallest id);
    two trees joined only by a pair stored as (hi, lo)"""
    rng = np.random.default_rng(3 + P)
    # the ruler path
    n = 160
    perm = rng.permutation(n).astype(np.int64)
    a, b, w = ruler_path(7)
    rows = rows_of(perm[a], perm[b], w)
    pp = build(lib, n, P, rows, rng)
    edges, weight, labels = pp.msf()
    expect(edges, weight, labels, rows, n, "ruler")
    c = pp.debug_msf_counters()
    assert int(c[0]) == 8 and int(c[4]) == 64 and int(c[5]) == 127 and int(c[6]) == n - 127, c
    assert model_rounds(rows[:, 0], rows[:, 1], rows[:, 2], n)[0] == [64, 32, 16, 8, 4, 2, 1]
    check(pp, f"ruler P={P}", rounds=7, isolated=n - 128)
    pp.close()
    # the ascending path
    n, L = 700, 600
    perm = rng.permutation(n).astype(np.int64)
    path = perm[:L]
    rows = rows_of(path[:-1], path[1:], np.arange(1, L))
    pp = build(lib, n, P, rows, rng)
    edges, weight, labels = pp.msf()
    expect(edges, weight, labels, rows, n, "ascending")
    assert weight == L * (L - 1) // 2
    c = pp.debug_msf_counters()
    assert int(c[0]) == 2 and int(c[4]) == L - 1 and int(c[3]) <= 11, c
    hooks, depth = model_rounds(rows[:, 0], rows[:, 1], rows[:, 2], n)
    assert hooks == [L - 1] and depth[0] >= L - 2  # ONE chain: every vertex hooks towards the light end (whose mutual pair keeps either root)
    check(pp, f"ascending P={P}")
    pp.close()
    # the star, half of it stored inward
    n, m = 600, 500
    perm = rng.permutation(n).astype(np.int64)
    hub, leaves = perm[0], perm[1:m + 1]
    rows = np.concatenate([rows_of(np.full(m // 2, hub), leaves[: m // 2], BIG), rows_of(leaves[m // 2:], np.full(m - m // 2, hub), BIG)])
    pp = build(lib, n, P, rows, rng)
    edges, weight, labels = pp.msf()
    expect(edges, weight, labels, rows, n, "star")
    assert weight == m * BIG and weight > 1 << 40
    assert int(pp.debug_msf_counters()[0]) == 2
    check(pp, f"star P={P}", ties=1, reverse_only=1)
    pp.close()
    # the complete graph, both directions stored for half of the pairs
    n, q = 100, 40
    perm = rng.permutation(n).astype(np.int64)
    kq = perm[:q]
    i, j = np.triu_indices(q, 1)
    rows = np.concatenate([rows_of(kq[i], kq[j], 1), rows_of(kq[j[::2]], kq[i[::2]], 1)])
    pp = build(lib, n, P, rows, rng)
    edges, weight, labels = pp.msf()
    least = int(kq.min())
    expect(edges, weight, labels, rows_of(np.full(q - 1, least), np.sort(kq)[1:], 1), n, "K_40")
    c = pp.debug_msf_counters()
    assert int(c[0]) == 2 and int(c[4]) == q - 1, c
    check(pp, f"K_40 P={P}", ties=q - 1)
    pp.close()
    # two paths and one pair between them, stored from the larger id to the smaller
    n = 300
    perm = rng.permutation(n).astype(np.int64)
    p1, p2 = perm[:100], perm[100:220]
    x, y = int(max(p1[50], p2[60])), int(min(p1[50], p2[60]))
    rows = np.concatenate([rows_of(p1[:-1], p1[1:], 1), rows_of(p2[:-1], p2[1:], 1), np.array([[x, y, 5]])])
    pp = build(lib, n, P, rows, rng)
    edges, weight, labels = pp.msf()
    expect(edges, weight, labels, rows, n, "joined")
    assert np.all(labels[np.concatenate([p1, p2])] == min(p1.min(), p2.min())) and weight == 99 + 119 + 5
    check(pp, f"joined P={P}", reverse_only=1)
    pp.close()


def test_sim_msf_invariant(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and one graph before and after a repartition that leaves a partition EMPTY: no output
    depends on the partitioning; P = 1 equals the partition's own engine call"""
    n = 1000
    ops = np.concatenate([zoo(streams, n, 10, 4000, seed=6), weigh(streams, mixed_stream(streams, n, seed=5), 6, seed=2)])
    results = []
    for P in (1, 2, 4, 8):
        pp = make(lib, n, P)
        pp.apply(ops)
        assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
        results.append(pp.msf())
        if P == 1:
            edges, weight, labels, ms = pp.partition(0).msf(with_ms=True)
            np.testing.assert_array_equal(edges, results[0][0])
            assert weight == results[0][1] and ms >= 0.0
            np.testing.assert_array_equal(labels, results[0][2])
            check(pp, "invariant", ties=1, opposite=1, reverse_only=1, loops=1, beyond=1, isolated=1, trees=2, rounds=2)
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
            tune(pp)
            assert all(last_slot_free(i) for _, i, _ in partition_states(pp))
            assert pp.partition(1).get_n() == 0
            results.append(check(pp, "empty partition", rounds=2)[:3])
        pp.close()
    for edges, weight, labels in results[1:]:
        np.testing.assert_array_equal(edges, results[0][0])
        assert weight == results[0][1]
        np.testing.assert_array_equal(labels, results[0][2])


@pytest.mark.parametrize("P,hub", [(1, 7), (3, 5990)])
def test_sim_msf_hub_and_long_list(lib, P, hub):
    """the hub graph of test_sim_kcore_hub_and_long_list with values: a hub with 5000 leaves and 60 neighbours in a clique
    K_100, its slot range longer than one wave walks.  The hub with a small id is the source of its stored pairs — whole
    waves on one source, reduced before the atomic — with a large id the destination of nearly all.  Leaf values 1 .. 3: the
    hub's component looks at 5000 cut edges for its lightest"""
    n = 6000
    rng = np.random.default_rng(P)
    others = rng.permutation(np.setdiff1d(np.arange(n), [hub]))
    leaves, kq = others[:5000], others[5000:5100]
    i, j = np.triu_indices(100, 1)
    pairs = np.concatenate([np.stack([np.full(5000, hub), leaves], axis=1), np.stack([kq[i], kq[j]], axis=1),
                            np.stack([np.full(60, hub), kq[:60]], axis=1)])
    ops = np.stack([pairs.min(axis=1), pairs.max(axis=1), rng.integers(1, 4, len(pairs))], axis=1).astype(np.uint32)
    ops = ops[rng.permutation(len(ops))]
    pp = make(lib, n, P)
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    if hub == 7:
        node = pp.getNode(hub)
        assert node[1] - node[0] > 4096
    edges, weight, labels, h = check(pp, f"hub P={P}", ties=50, isolated=1)
    assert len(edges) == 5100 and int(((edges[:, 0] == hub) | (edges[:, 1] == hub)).sum()) >= 5001
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_msf_answers_in_the_sequential_regime(lib, streams, P):
    """narrow == 0 on one partition: the call is not refused (it intersects nothing) and equals the model"""
    n = 500
    pp = make(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 9, 3000, seed=23)
    adds = weigh(streams, streams.adds(s, d), 4, seed=9)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    e = pp.partition(P - 1)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    tri = np.empty(n, np.uint64)
    assert pp.L.pppcsr_triangles(pp.h, tri.ctypes.data, None, None) == EUNSUPPORTED  # (the regime is the one triangles refuses)
    check(pp, f"sequential P={P}", ties=1, reverse_only=1)
    edges, weight, labels = e.msf()
    assert len(labels) == e.get_n()
    assert e.stats()["narrow"] == 0
    pp.close()


def test_sim_msf_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    L, h = pp.L, pp.h
    e = pp.partition(0)
    edges = np.full((n, 3), 77, np.uint32)
    labels = np.full(n, 77, np.uint32)
    count, weight = ctypes.c_uint64(77), ctypes.c_uint64(77)
    ms = ctypes.c_double()
    # n vertices and no edge
    assert L.pppcsr_msf(h, edges.ctypes.data, n, ctypes.byref(count), ctypes.byref(weight), labels.ctypes.data, None) == 0
    assert count.value == 0 and weight.value == 0 and np.array_equal(labels, np.arange(n)) and np.all(edges == 77)
    assert pp.debug_msf_counters().tolist() == [1, 1, 0, 0, 0, 0, n, 2]
    # n = 0
    z = pkg.PCSR(0, lib=lib)
    got_e, got_w, got_l = z.msf()
    assert got_e.shape == (0, 3) and got_w == 0 and len(got_l) == 0
    assert not z.debug_msf_counters().any()
    pp.apply(weigh(streams, streams.random_stream(n, 900, seed=1), 5, seed=3))
    want_e, want_w, want_l = model_msf(*global_edges_valued(partition_states(pp)), n)
    assert len(want_e) >= 100
    for fn, hh, m in ((L.pppcsr_msf, h, n), (L.ppcsr_msf, e.h, e.get_n())):
        assert fn(hh, None, 0, None, None, None, None) == EINVAL
        assert fn(hh, None, 5, None, None, None, ctypes.byref(ms)) == EINVAL  # all four outputs NULL
        assert fn(None, edges.ctypes.data, n, ctypes.byref(count), ctypes.byref(weight), labels.ctypes.data, None) == EINVAL
        count.value = weight.value = 77
        assert fn(hh, None, 0, ctypes.byref(count), None, None, None) == 0 and count.value != 77  # each output alone
        total = count.value
        assert fn(hh, None, 0, None, ctypes.byref(weight), None, ctypes.byref(ms)) == 0 and weight.value != 77 and ms.value >= 0.0
        labels[:] = 77
        assert fn(hh, None, 0, None, None, labels.ctypes.data, None) == 0
        assert int((labels[:m] == np.arange(m)).sum()) == m - total and np.all(labels[m:] == 77)
        edges[:] = 77
        assert fn(hh, edges.ctypes.data, n, None, None, None, None) == 0
        assert np.all(edges[:total, 0] < edges[:total, 1]) and int(edges[:total, 2].sum()) == weight.value and np.all(edges[total:] == 77)
    # ERANGE: the first cap edges are written, *count is the needed size, the other outputs are delivered
    full = len(want_e)
    edges[:] = 77
    labels[:] = 77
    count.value = weight.value = 77
    assert L.pppcsr_msf(h, edges.ctypes.data, full - 1, ctypes.byref(count), ctypes.byref(weight), labels.ctypes.data, None) == ERANGE
    assert count.value == full and weight.value == want_w
    np.testing.assert_array_equal(edges[: full - 1].astype(np.int64), want_e[: full - 1])
    assert np.all(edges[full - 1:] == 77)
    np.testing.assert_array_equal(labels, want_l)
    assert L.pppcsr_msf(h, edges.ctypes.data, 0, ctypes.byref(count), None, None, None) == ERANGE and count.value == full
    assert L.pppcsr_msf(h, edges.ctypes.data, full, ctypes.byref(count), None, None, None) == 0
    np.testing.assert_array_equal(edges[:full].astype(np.int64), want_e)
    assert L.ppcsr_debug_msf_counters(None, edges.ctypes.data) == EINVAL
    assert L.ppcsr_debug_msf_counters(e.h, None) == EINVAL
    out = np.zeros(8, np.uint64)
    assert L.ppcsr_debug_msf_counters(e.h, out.ctypes.data) == 0 and int(out[5]) == full
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_msf(loc.h, edges.ctypes.data, n, ctypes.byref(count), None, None, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one)
    pp.close()


def test_sim_msf_allocation_failures(lib, streams):
    """every device allocation of the call fails in turn: the allocation status comes back, the state is unchanged, and the
    next call succeeds and equals the model"""
    def prepare(pp, states):
        n = pp.get_n()
        src, dst, val = global_edges_valued(states)
        want_e, want_w, want_l = model_msf(src, dst, val, n)
        edges = np.empty((n, 3), np.uint32)
        labels = np.empty(n, np.uint32)
        count, weight = ctypes.c_uint64(), ctypes.c_uint64()

        def verify(k):
            got_e, got_w, got_l = pp.msf()
            np.testing.assert_array_equal(got_e.astype(np.int64), want_e)
            assert got_w == want_w
            np.testing.assert_array_equal(got_l, want_l)
        return (lambda k: pp.L.pppcsr_msf(pp.h, edges.ctypes.data, n, ctypes.byref(count), ctypes.byref(weight), labels.ctypes.data, None),
                lambda k: EHIP, verify)
    for P in (1, 3):
        # the table, comp, parents, best weights, best pairs, two key lists, two weight lists, the packed edges, the counters, the length
        alloc_failures(lib, streams, P, prepare, 12)
