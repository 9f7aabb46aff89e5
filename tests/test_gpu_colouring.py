"""GPU: ppcsr_colouring / ppcsr_mis and their pppcsr_ forms on MI355X, all partitions on one device: against the models of
tests/colouring_model.py (sequential greedy on Python integers where the size allows, the synchronous numpy replicas of the
rounds everywhere) and its order-blind validators — at RMAT scale 14 under streams and a repartition, once at scale 18 on 8
partitions and on one PCSR, at the grid-stride seams of the vertex launches and of the streaming pass, on the hub graph with a
64-colour window, and over a few rounds of batch-then-check."""
import ctypes

import numpy as np
import pytest

from colouring_model import (WAVE_SLOTS, assert_hard, assert_maximal_independent, assert_proper, graph, hardness, levels, mis_rounds,
                             model_colouring, model_mis)
from consumers_model import global_edges, partition_states
from helpers import load_pkg

pytestmark = pytest.mark.gpu
ORDERS = ("random", "degree", "id")
STREAM_GRID_SLOTS = 1 << 23  # slots one step of a streaming pass covers: its grid stops growing at 8192 workgroups of 1024 slots
VERTEX_GRID = 1 << 20        # vertices one step of a vertex launch covers: 4096 workgroups of 256 threads
LIST_GRID_WAVES = 1 << 16    # frontier vertices one step of a round covers: 16384 workgroups of four waves


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


def model(src, dst, n, order, seed, python_loops):
    rows, nbr, keys, rank = graph(src, dst, n, ORDERS.index(order), seed)
    _, sizes, colour = levels(rows, nbr, rank)
    mask, rounds = mis_rounds(src, dst, n, rank)
    if python_loops:  # the definitions themselves, beside the synchronous replicas
        np.testing.assert_array_equal(colour, model_colouring(rows, nbr, keys))
        np.testing.assert_array_equal(mask, model_mis(rows, nbr, keys))
    return rows, nbr, colour, mask, sizes, rounds


def compare_mis(g, rows, nbr, want_mask, rounds, order, seed, label):
    mask, size, ms = g.mis(order, seed, with_ms=True)
    m = g.debug_mis_counters()
    print(f"{label}: mis {ms:.3f} ms, counters {m.tolist()}")
    np.testing.assert_array_equal(mask, want_mask, err_msg=f"{label}: in_set")
    assert size == rounds["size"] and ms >= 0.0
    assert (m[0], m[1], m[2], m[3], m[4], m[5]) == (rounds["rounds"], rounds["rounds"], rounds["members1"], rounds["undecided1"],
                                                    rounds["size"], 1 if order == "degree" else 0), (label, m, rounds)
    assert_maximal_independent(rows, nbr, mask, label)
    return mask


def compare(g, src, dst, n, order, seed, label, python_loops=True, **hard):
    """one colouring and one mis call against the model: arrays, totals, the counters that are functions of the graph and the
    order, in_set == (colour == 0), the validators; the conditions on the input first, from the model"""
    rows, nbr, want, want_mask, sizes, rounds = model(src, dst, n, order, seed, python_loops)
    h = hardness(src, dst, n, rows, want, sizes)
    h["mis_rounds"] = rounds["rounds"]
    assert_hard(h, label, **hard)
    colour, ncolours, ms = g.colouring(order, seed, with_ms=True)
    c = g.debug_colouring_counters()
    print(f"{label}: colouring {ms:.3f} ms, counters {c.tolist()}")
    np.testing.assert_array_equal(colour, want, err_msg=f"{label}: colour")
    assert ncolours == h["ncolours"] and ms >= 0.0, (label, ncolours, h)
    assert (c[0], c[1], c[2], c[3], c[4]) == (h["rounds"], h["widest"], h["long_lists"], 2 * h["edges"], h["ncolours"]), (label, c, h)
    mask = compare_mis(g, rows, nbr, want_mask, rounds, order, seed, label)
    np.testing.assert_array_equal(mask, colour == 0, err_msg=label)
    assert_proper(rows, nbr, colour, label)
    return colour, mask, h


def check_model(pp, label, orders=ORDERS, seed=7, python_loops=True, **hard):
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    out = {order: compare(pp, src, dst, n, order, seed, f"{label} {order}", python_loops, **hard) for order in orders}
    for (_, i0, n0), (_, i1, n1) in zip(states, partition_states(pp)):  # nothing written
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1), label
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return out


def test_colouring_model_rmat14(pkg, streams):
    """P = 8: an RMAT core, a mixed stream over stored and fresh pairs with destinations >= n, add_node and edges to and from
    the new vertex, a repartition to balanced_starts; the three orders"""
    n, P = 1 << 14, 8
    hard = dict(ncolours=16, rounds=64, mis_rounds=6, widest=4096, maxdeg=1000, backward=1, loops=1, beyond=1)
    s, d = streams.rmat_edges(14, 120_000, seed=51)
    core = streams.adds(s, d)
    s2, d2 = streams.rmat_edges(14, 2_000, seed=52)
    mixed = streams.mixed_existing_stream(core, streams.adds(s2, d2 + np.uint32(7)), seed=53)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    pp.apply(core)
    pp.apply(mixed)
    check_model(pp, "rmat14", **hard)
    pp.add_node()
    pp.apply(np.array([[n, 1, 5], [2, n, 9], [1, n, 1], [0, n, 1], [1, 2, 1]], np.uint32))
    pp.add_node()  # (isolated unless the stream named it)
    out = check_model(pp, "rmat14 add_node", orders=("id", "random"), **hard)
    assert out["id"][0][n] >= 1  # (0, 1 and 2 precede it)
    pp.repartition(pp.balanced_starts())
    check_model(pp, "rmat14 repartitioned", orders=("degree",), **hard)
    pp.close()


def test_colouring_model_rmat18(pkg, streams):
    """once at scale 18, bulk-built from a device tensor on 8 partitions and on one PCSR, random and degree orders: a first
    frontier beyond the list grid's 65536 waves, a list beyond one wave's reach, hundreds of rounds.  The floors on the input
    are rounded down from what the host model shows for it (random / degree: 371 / 349 colouring rounds, 69 / 47 colours, a
    widest frontier of 174088 / 141599, 11 / 22 MIS rounds; largest degree 9192)"""
    n = 1 << 18
    s, d = streams.rmat_edges(18, 2_000_000, seed=31)
    adds = streams.adds(s, d)
    t = to_device(adds)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    pp.bulk_build_device(t.data_ptr(), len(adds))
    one = pkg.PCSR(n)
    one.bulk_build(adds)
    del t
    key = np.unique(adds[:, 0].astype(np.int64) * n + adds[:, 1].astype(np.int64))  # (the distinct pairs a bulk build stores)
    src, dst = key // n, key % n
    floors = dict(random=dict(rounds=256, ncolours=64, mis_rounds=8), degree=dict(rounds=256, ncolours=40, mis_rounds=16))
    for order in ("random", "degree"):
        colour, mask, h = compare(pp, src, dst, n, order, 3, f"rmat18 {order}", python_loops=False, maxdeg=WAVE_SLOTS + 1,
                                  long_lists=1, widest=LIST_GRID_WAVES + 1, **floors[order])
        got, ncolours = one.colouring(order, 3)
        np.testing.assert_array_equal(got, colour)
        assert ncolours == h["ncolours"]
        got, size = one.mis(order, 3)
        np.testing.assert_array_equal(got, mask)
        assert size == mask.sum()
    pp.close()
    one.close()


def test_colouring_vertex_grid_stride(pkg):
    """n = 2^20 + 777 with a sparse edge set (a random permutation's path broken every 16 vertices, and a few chords): the
    vertex launches stride, and the tail past 2^20 is part of the graph"""
    n = VERTEX_GRID + 777
    rng = np.random.default_rng(4)
    perm = rng.permutation(n).astype(np.int64)
    a, b = perm[:-1], perm[1:]
    keep = np.arange(n - 1) % 16 != 15
    ca, cb = rng.integers(0, n, 200_000), rng.integers(0, n, 200_000)
    key = np.unique(np.minimum(np.concatenate([a[keep], ca]), np.concatenate([b[keep], cb])) * n
                    + np.maximum(np.concatenate([a[keep], ca]), np.concatenate([b[keep], cb])))
    key = key[key // n != key % n]
    adds = np.stack([key // n, key % n, np.ones(len(key), np.int64)], axis=1).astype(np.uint32)
    g = pkg.PCSR(n)
    g.bulk_build(adds[rng.permutation(len(adds))])
    src, dst = adds[:, 0].astype(np.int64), adds[:, 1].astype(np.int64)
    for order in ("random", "id"):
        colour, mask, _ = compare(g, src, dst, n, order, 1, f"vertex stride {order}", python_loops=False, ncolours=4, rounds=4, widest=VERTEX_GRID // 4)
        assert colour[VERTEX_GRID:].max() >= 1 and mask[VERTEX_GRID:].any() and not mask[VERTEX_GRID:].all()
    g.close()


def test_mis_pass_grid_stride(pkg):
    """MIS only, on arrays of more than 2^23 slots: the streaming pass's grid has stopped growing and every wave loops.
    n = 2^19, 14 pairs per vertex inside blocks of 64 consecutive ids; against the numpy replica of the rounds"""
    n, B = 1 << 19, 64
    rng = np.random.default_rng(9)
    v = np.repeat(np.arange(n, dtype=np.int64), 14)
    w = v - v % B + rng.integers(0, B, len(v))
    key = np.unique(v * n + w)  # (a bulk build takes distinct pairs)
    adds = np.stack([key // n, key % n, np.ones(len(key), np.int64)], axis=1).astype(np.uint32)
    g = pkg.PCSR(n)
    g.bulk_build(adds[rng.permutation(len(adds))])
    slots = g.geometry()[0]
    assert slots > STREAM_GRID_SLOTS, slots
    src, dst = adds[:, 0].astype(np.int64), adds[:, 1].astype(np.int64)
    rows, nbr, keys, rank = graph(src, dst, n, 0, 6)
    want, rounds = mis_rounds(src, dst, n, rank)
    assert rounds["rounds"] >= 4 and (src > dst).any() and (src == dst).any()
    compare_mis(g, rows, nbr, want, rounds, "random", 6, "pass stride")
    g.close()


def hub_graph(n, hub, rng):
    others = rng.permutation(np.setdiff1d(np.arange(n), [hub]))
    leaves, kq = others[:5000], others[5000:5100]
    i, j = np.triu_indices(100, 1)
    pairs = np.concatenate([np.stack([np.full(5100, hub), others[:5100]], axis=1), np.stack([kq[i], kq[j]], axis=1)])
    return np.stack([pairs.min(axis=1), pairs.max(axis=1), np.ones(len(pairs), np.int64)], axis=1).astype(np.uint32)


def test_colouring_window_on_the_hub_graph(pkg):
    """a hub (largest id) with 5000 leaves that is adjacent to all of K_100, under `id`: the long-list kernel decides colour
    100; with colour_window = 64 it needs a second window, counter [5], and gives the same"""
    n, hub = 6000, 5999
    rng = np.random.default_rng(5)
    ops = hub_graph(n, hub, rng)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=2)
    pp.apply(ops[rng.permutation(len(ops))])
    src, dst = global_edges(partition_states(pp))
    colour, _, _ = compare(pp, src, dst, n, "id", 0, "default window", long_lists=1, ncolours=101)
    assert colour[hub] == 100 and pp.debug_colouring_counters()[5] == 0
    pp.partition(0).set_option("colour_window", 64)
    narrow, _, _ = compare(pp, src, dst, n, "id", 0, "window 64")
    np.testing.assert_array_equal(narrow, colour)
    assert pp.debug_colouring_counters()[5] == 1 and pp.debug_colouring_counters()[2] == 1
    compare(pp, src, dst, n, "degree", 2, "window 64, degree")
    pp.close()


def test_colouring_follow_batches(pkg, streams):
    """3 rounds of: apply a batch of adds, deletes, a self-loop and a destination >= n, then both calls against the model"""
    n, P = 1 << 14, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges(14, 60_000, seed=61)
    pp.apply(streams.adds(s, d))
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 20_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 10_000, seed=80 + r, p_delete=0.5),
                                np.array([[r, r, 1], [r, n + r, 1]], np.uint32)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        check_model(pp, f"round {r}", orders=(ORDERS[r],), seed=r, ncolours=12, rounds=32, backward=1, loops=1, beyond=1)
    pp.close()


def test_colouring_status_codes(pkg, streams):
    """argument errors with EINVAL; partitions on two devices refused with EUNSUPPORTED; the sequential regime answered"""
    n = 1 << 12
    s, d = streams.rmat_edges(12, 60_000, seed=41)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4)
    pp.apply(streams.adds(s, d))
    L = pp.L
    colour, member = np.empty(n, np.uint32), np.empty(n, np.uint8)
    ncol, size = ctypes.c_uint32(77), ctypes.c_uint64(77)
    e = pp.partition(2)
    for col, mis, h in ((L.pppcsr_colouring, L.pppcsr_mis, pp.h), (L.ppcsr_colouring, L.ppcsr_mis, e.h)):
        assert col(h, 0, 1, None, None, None) == 1 and mis(h, 0, 1, None, None, None) == 1
        assert col(None, 0, 1, colour.ctypes.data, ctypes.byref(ncol), None) == 1
        assert mis(None, 0, 1, member.ctypes.data, ctypes.byref(size), None) == 1
        assert col(h, 3, 1, colour.ctypes.data, ctypes.byref(ncol), None) == 1
        assert mis(h, 0xFFFFFFFF, 1, member.ctypes.data, ctypes.byref(size), None) == 1
    assert L.ppcsr_set_option(e.h, b"colour_window", 96) == 1 and L.ppcsr_set_option(e.h, b"colour_window", 32768) == 0
    src, dst = global_edges(partition_states(pp))
    _, _, want, want_mask, _, _ = model(src, dst, n, "degree", 1, True)
    assert L.pppcsr_colouring(pp.h, 1, 1, None, ctypes.byref(ncol), None) == 0 and ncol.value == want.max() + 1 >= 16
    assert L.pppcsr_mis(pp.h, 1, 1, None, ctypes.byref(size), None) == 0 and size.value == want_mask.sum()
    assert L.pppcsr_colouring(pp.h, 1, 1, colour.ctypes.data, None, None) == 0
    assert L.pppcsr_mis(pp.h, 1, 1, member.ctypes.data, None, None) == 0
    np.testing.assert_array_equal(colour, want)
    np.testing.assert_array_equal(member.astype(bool), want_mask)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    tri = np.empty(n, np.uint64)
    assert L.pppcsr_triangles(pp.h, tri.ctypes.data, None, None) == 4  # (the regime triangles refuses)
    np.testing.assert_array_equal(pp.colouring("degree", 1)[0], want)
    np.testing.assert_array_equal(pp.mis("degree", 1)[0], want_mask)
    assert len(e.colouring()[0]) == e.get_n() and len(e.mis()[0]) == e.get_n()
    e.set_option("search_narrow", 1)
    if L.ppcsr_device_count() >= 2:
        two = pkg.PPPCSR(n, numDomain=2, partitionsPerDomain=1, devices=[0, 1])
        assert L.pppcsr_colouring(two.h, 0, 1, colour.ctypes.data, ctypes.byref(ncol), None) == 4
        assert "more than one device" in L.ppcsr_last_error().decode()
        assert L.pppcsr_mis(two.h, 0, 1, member.ctypes.data, ctypes.byref(size), None) == 4
        assert "more than one device" in L.ppcsr_last_error().decode()
    pp.close()
