"""CPU: ppcsr_colouring / ppcsr_mis and their pppcsr_ forms on the fiber SIMT emulator (tests/hostsim), which compiles the engine's
own kernel and host source.  Results and every graph-determined counter are checked exactly against tests/colouring_model.py
(sequential greedy on Python integers, and synchronous numpy replicas of the rounds beside it), built from the exported partition
states, against order-blind validators and against closed forms."""
import ctypes

import numpy as np
import pytest

from colouring_model import (WAVE_SLOTS, assert_hard, assert_maximal_independent, assert_proper, graph, hardness, levels, mis_rounds,
                             model_colouring, model_mis)
from consumers_model import global_edges, last_slot_free, partition_states
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim
from test_sim_kcore import alloc_failures
from test_sim_pppcsr_consumers import make, mixed_stream, tune

EINVAL, ENOMEM, EHIP, EUNSUPPORTED = 1, 2, 3, 4
ORDERS = ("random", "degree", "id")


@pytest.fixture(scope="module")
def lib():
    build_sim()
    L = load_pkg().load_library(SIM_SO)
    L.ppcsr_sim_fail_alloc_after.argtypes = [ctypes.c_int]
    return L


def model(src, dst, n, order, seed, python_loops=True):
    """everything the device must reproduce for one order and seed"""
    rows, nbr, keys, rank = graph(src, dst, n, ORDERS.index(order), seed)
    _, sizes, colour = levels(rows, nbr, rank)
    mask, rounds = mis_rounds(src, dst, n, rank)
    if python_loops:  # the definitions themselves, beside the synchronous replicas
        np.testing.assert_array_equal(colour, model_colouring(rows, nbr, keys))
        np.testing.assert_array_equal(mask, model_mis(rows, nbr, keys))
    return rows, nbr, colour, mask, sizes, rounds


def compare(pp, src, dst, n, order, seed, label):
    """one colouring and one mis call against the model: arrays, totals, the counters that are functions of the graph and
    the order, in_set == (colour == 0), the validators"""
    rows, nbr, want, want_mask, sizes, rounds = model(src, dst, n, order, seed)
    h = hardness(src, dst, n, rows, want, sizes)
    colour, ncolours, ms = pp.colouring(order, seed, with_ms=True)
    np.testing.assert_array_equal(colour, want, err_msg=f"{label}: colour")
    assert ncolours == h["ncolours"] and ms >= 0.0, (label, ncolours, h)
    c = pp.debug_colouring_counters()
    assert (c[0], c[1], c[2], c[3], c[4]) == (h["rounds"], h["widest"], h["long_lists"], 2 * h["edges"], h["ncolours"]), (label, c, h)
    assert c[6] >= c[0] and c[7] >= c[0], (label, c)
    mask, size, ms = pp.mis(order, seed, with_ms=True)
    np.testing.assert_array_equal(mask, want_mask, err_msg=f"{label}: in_set")
    m = pp.debug_mis_counters()
    assert size == rounds["size"] and ms >= 0.0
    assert (m[0], m[1], m[2], m[3], m[4], m[5]) == (rounds["rounds"], rounds["rounds"], rounds["members1"], rounds["undecided1"],
                                                    rounds["size"], 1 if order == "degree" else 0), (label, m, rounds)
    assert m[6] >= 2 * m[0] and m[7] == m[0], (label, m)
    np.testing.assert_array_equal(mask, colour == 0, err_msg=label)
    assert_proper(rows, nbr, colour, label)
    assert_maximal_independent(rows, nbr, mask, label)
    return colour, mask, h, rounds


def check(pp, label, orders=ORDERS, seeds=(0, 77), **hard):
    """every order and seed against the model, the conditions on the input from the model; nothing written (states and stats)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    out = {}
    for order in orders:
        for seed in (seeds if order != "id" else seeds[:1]):
            out[order, seed] = compare(pp, src, dst, n, order, seed, f"{label} {order} seed={seed}")
            assert_hard(out[order, seed][2], f"{label} {order}", **hard)
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return out


def upper(pairs):
    """rows (min, max, 1) of undirected pairs"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.stack([p.min(axis=1), p.max(axis=1), np.ones(len(p), np.int64)], axis=1).astype(np.uint32)


def clique(ids):
    ids = np.asarray(ids)
    i, j = np.triu_indices(len(ids), 1)
    return np.stack([ids[i], ids[j]], axis=1)


def star(hub, leaves):
    leaves = np.asarray(leaves)
    return np.stack([np.full(len(leaves), hub), leaves], axis=1)


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_colouring_model(lib, streams, P):
    """a bulk-built folded RMAT core under a mixed stream (deletes, duplicate adds, destinations >= n), add_node twice and
    edges to and from the new vertices, a repartition to balanced_starts.  P = 3 runs with every wv::uni / wv::bcast verified"""
    n = 1200
    hard = dict(ncolours=8, rounds=6, widest=100, maxdeg=65, isolated=1, backward=1, loops=1, beyond=1)
    lib.ppcsr_sim_check_uniform(1 if P == 3 else 0)
    try:
        pp = make(lib, n, P)
        s, d = streams.rmat_edges_folded(n, 11, 8000, seed=41)
        adds = np.concatenate([streams.adds(s, d), np.array([[5, 5, 1]], np.uint32)])
        pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
        ops = mixed_stream(streams, n, seed=40 + P)
        pp.apply(ops[: len(ops) // 2])
        pp.apply(ops[len(ops) // 2:])
        check(pp, f"P={P}", **hard)
        pp.add_node()
        pp.add_node()
        pp.apply(np.array([[n, 3, 2], [7, n, 3], [3, n, 1], [9, n, 1], [n, n + 1, 1], [n + 5, 1, 1], [n + 1, n + 9, 1]], np.uint32))
        out = check(pp, f"P={P} add_node", **hard)
        colour = out["id", 0][0]
        assert colour[n] >= 1 and colour[n + 1] == (1 if colour[n] == 0 else 0)  # (n: neighbours 3, 7, 9 before it; n + 1: only n)
        pp.repartition(pp.balanced_starts())
        tune(pp)
        check(pp, f"P={P} repartitioned", **hard)
        pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


@pytest.mark.parametrize("P", [1, 4])
def test_sim_colouring_closed_forms(lib, P):
    """K_30 (30 distinct colours under every order), a tree and an even cycle (two colours under random orders at least, the
    members an independent dominating set) and isolated vertices (colour 0, members) on permuted ids in one shuffled stream;
    then the orientation convention"""
    n = 400
    rng = np.random.default_rng(3 + P)
    perm = rng.permutation(n)
    kq, cyc, tree, lone = perm[:30], perm[30:80], perm[80:200], perm[200:]
    pairs = [clique(kq), np.stack([cyc, np.roll(cyc, -1)], axis=1),
             np.array([[tree[i], tree[rng.integers(0, i)]] for i in range(1, len(tree))])]
    ops = upper(np.concatenate(pairs))
    ops = ops[rng.permutation(len(ops))]
    pp = make(lib, n, P)
    pp.apply(ops)
    first = {}
    for order in ORDERS:
        colour, ncolours = pp.colouring(order, 9)
        mask, size = pp.mis(order, 9)
        assert sorted(colour[kq].tolist()) == list(range(30)) and ncolours == 30
        assert not colour[lone].any() and mask[lone].all()
        assert colour[tree].max() >= 1 and colour[cyc].max() in (1, 2) and mask[kq].sum() == 1
        assert size == mask.sum()
        first[order] = (colour, mask)
    check(pp, f"closed P={P}", ncolours=30, isolated=len(lone))
    # a self-loop, a destination >= n and backward pairs (between isolated vertices, and inside the tree) change nothing
    a, b = sorted(int(x) for x in lone[:2])
    pp.apply(np.array([[a, a, 1], [a, n + 3, 1], [b, a, 1], [max(tree[0], tree[5]), min(tree[0], tree[5]), 1]], np.uint32))
    for order in ORDERS:
        colour, _ = pp.colouring(order, 9)
        mask, _ = pp.mis(order, 9)
        np.testing.assert_array_equal(colour, first[order][0])
        np.testing.assert_array_equal(mask, first[order][1])
    check(pp, f"closed P={P} + no-ops", backward=2, loops=1, beyond=1)
    # both directions stored: the same as the upper triangle alone
    pp.apply(ops[:, [1, 0, 2]])
    for order in ORDERS:
        np.testing.assert_array_equal(pp.colouring(order, 9)[0], first[order][0])
        np.testing.assert_array_equal(pp.mis(order, 9)[0], first[order][1])
    pp.close()


@pytest.mark.parametrize("P", [1, 4])
def test_sim_colouring_first_fit_worst_cases(lib, P):
    """under `id`: the crown graph on 2 x 20 interleaved vertices takes 20 colours where two suffice; the path 0 - 1 - ... - 599
    on its natural ids alternates 0 / 1 over 600 colouring rounds and its MIS is the even vertices, after 600 rounds too"""
    m, L = 20, 600
    n = 2 * m + L
    ai, bj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    keep = ai != bj
    crown = np.stack([2 * ai[keep], 2 * bj[keep] + 1], axis=1)
    path = np.stack([np.arange(L - 1), np.arange(1, L)], axis=1) + 2 * m
    ops = upper(np.concatenate([crown, path]))
    pp = make(lib, n, P)
    pp.apply(ops[np.random.default_rng(P).permutation(len(ops))])
    colour, ncolours = pp.colouring("id")
    np.testing.assert_array_equal(colour[:2 * m], np.arange(2 * m) // 2)
    np.testing.assert_array_equal(colour[2 * m:], np.arange(L) % 2)
    assert ncolours == m
    c = pp.debug_colouring_counters()
    assert c[0] == L and c[4] == m
    mask, size = pp.mis("id")
    np.testing.assert_array_equal(mask[2 * m:], np.arange(L) % 2 == 0)
    assert mask[:2 * m].sum() == 2 and size == L // 2 + 2
    assert pp.debug_mis_counters()[0] == L
    check(pp, f"worst P={P}", orders=("id", "random"), seeds=(4,))
    pp.close()


def hub_graph(n, hub, rng, all_of_clique=False):
    """test_sim_kcore_hub_and_long_list's: 5000 leaves and K_100, 60 (or all) of whose members are adjacent to the hub"""
    others = rng.permutation(np.setdiff1d(np.arange(n), [hub]))
    leaves, kq = others[:5000], others[5000:5100]
    return leaves, kq, upper(np.concatenate([star(hub, leaves), clique(kq), star(hub, kq if all_of_clique else kq[:60])]))


@pytest.mark.parametrize("P,hub", [(1, 0), (3, 5999)])
def test_sim_colouring_hub_and_long_list(lib, P, hub):
    """a hub with 5060 neighbours, a list beyond what one wave walks.  With the smallest id it precedes them all under `id`:
    colour 0, and the long kernel makes its 5060 decrements, which release a frontier of 5000 leaves at once.  With the
    largest id every neighbour precedes it and the long kernel decides its colour from 5060 coloured entries"""
    n = 6000
    rng = np.random.default_rng(P)
    leaves, kq, ops = hub_graph(n, hub, rng)
    pp = make(lib, n, P)
    ops = ops[rng.permutation(len(ops))]
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    out = check(pp, f"hub P={P}", seeds=(3,), maxdeg=WAVE_SLOTS + 1, long_lists=1, ncolours=100)
    colour, mask, h, _ = out["id", 3]
    assert h["maxdeg"] == 5060
    if hub == 0:
        assert colour[hub] == 0 and mask[hub] and colour[leaves].min() == 1 and h["widest"] >= 5000
    else:
        assert not colour[leaves].any() and colour[hub] >= 1 and not mask[hub]
    pp.close()


@pytest.mark.parametrize("hubs_first", [False, True])
def test_sim_colouring_list_length_seams(lib, hubs_first):
    """hubs with exactly 64 / 65 neighbours (the seam between a walk that stays in registers and one that uses LDS), 4096 / 4097
    (between the wave's walk and the long kernel) and 2 x 4096 + 1 — adjacent to whole cliques, so that the forbidden sets are
    full up to 64, 65 and 100.  Under `id` with the hubs last their colours are closed forms; with the hubs first they precede
    every neighbour"""
    sizes = {"h64": 0, "h65": 0, "h4096": 3996, "h4097": 3997, "h8193": 8093}
    n = 17000
    shift = 5 if hubs_first else 0
    hub = {name: (i if hubs_first else n - 5 + i) for i, name in enumerate(sizes)}
    c100, c64, c65 = np.arange(0, 100) + shift, np.arange(100, 164) + shift, np.arange(164, 229) + shift
    pairs = [clique(c100), clique(c64), clique(c65), star(hub["h64"], c64), star(hub["h65"], c65)]
    at = 300
    for name in ("h4096", "h4097", "h8193"):
        pairs += [star(hub[name], c100), star(hub[name], np.arange(at, at + sizes[name]))]
        at += sizes[name]
    ops = upper(np.concatenate(pairs))
    pp = make(lib, n, 2)
    ops = ops[np.random.default_rng(8).permutation(len(ops))]
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    src, dst = global_edges(partition_states(pp))
    deg = np.bincount(np.concatenate([ops[:, 0], ops[:, 1]]), minlength=n)
    assert [int(deg[hub[k]]) for k in sizes] == [64, 65, 4096, 4097, 8193]
    colour, _, h, _ = compare(pp, src, dst, n, "id", 0, f"seams first={hubs_first}")
    assert h["long_lists"] == 2
    want = [0] * 5 if hubs_first else [64, 65, 100, 100, 100]
    assert [int(colour[hub[k]]) for k in sizes] == want
    compare(pp, src, dst, n, "random", 12, f"seams first={hubs_first}")
    compare(pp, src, dst, n, "degree", 12, f"seams first={hubs_first}")
    pp.close()


def test_sim_colouring_window(lib):
    """colour_window = 64 on a hub (largest id, 5100 neighbours) adjacent to all of K_100: the window of colours 0 .. 63 is full,
    the second one holds the answer — counter [5] counts the extra pass — and the result equals the default window's"""
    n, hub = 6000, 5999
    rng = np.random.default_rng(5)
    leaves, kq, ops = hub_graph(n, hub, rng, all_of_clique=True)
    pp = make(lib, n, 2)
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    src, dst = global_edges(partition_states(pp))
    colour, _, _, _ = compare(pp, src, dst, n, "id", 0, "default window")
    assert colour[hub] == 100 and pp.debug_colouring_counters()[5] == 0
    pp.partition(0).set_option("colour_window", 64)
    narrow, _, _, _ = compare(pp, src, dst, n, "id", 0, "window 64")
    np.testing.assert_array_equal(narrow, colour)
    assert pp.debug_colouring_counters()[5] == 1 and pp.debug_colouring_counters()[2] == 1
    compare(pp, src, dst, n, "degree", 2, "window 64, degree")
    pp.close()


def test_sim_colouring_invariant(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and one graph before and after a repartition with an empty partition: equal results;
    P = 1 equals the partition's own engine call"""
    n = 1000
    s, d = streams.rmat_edges_folded(n, 10, 5000, seed=6)
    adds, ops = streams.adds(s, d), mixed_stream(streams, n, seed=5)
    results = []

    def both(x):
        return [x.colouring(o, 21) for o in ORDERS] + [x.mis(o, 21) for o in ORDERS]
    for P in (1, 2, 4, 8):
        pp = make(lib, n, P)
        pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
        pp.apply(ops)
        assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
        results.append(both(pp))
        if P == 1:
            results.append(both(pp.partition(0)))
            check(pp, "invariant", seeds=(21,), ncolours=6)
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
            tune(pp)
            results.append(both(pp))
        pp.close()
    for r in results[1:]:
        for (x, kx), (y, ky) in zip(r, results[0]):
            np.testing.assert_array_equal(x, y)
            assert kx == ky


@pytest.mark.parametrize("P", [1, 3])
def test_sim_colouring_answers_in_the_sequential_regime(lib, streams, P):
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
    check(pp, f"sequential P={P}", seeds=(1,), ncolours=6)
    assert len(e.colouring()[0]) == e.get_n() and len(e.mis()[0]) == e.get_n()
    assert e.stats()["narrow"] == 0
    pp.close()


def test_sim_colouring_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    L, h = pp.L, pp.h
    e = pp.partition(0)
    colour = np.full(n, 77, np.uint32)
    member = np.full(n, 77, np.uint8)
    ncol, size, ms = ctypes.c_uint32(77), ctypes.c_uint64(77), ctypes.c_double()
    # n vertices and no edge: colour 0 everywhere, one colour, every vertex a member
    assert L.pppcsr_colouring(h, 0, 1, colour.ctypes.data, ctypes.byref(ncol), None) == 0
    assert not colour.any() and ncol.value == 1
    assert L.pppcsr_mis(h, 1, 1, member.ctypes.data, ctypes.byref(size), None) == 0
    assert np.all(member == 1) and size.value == n
    assert list(pp.debug_colouring_counters()[:5]) == [1, n, 0, 0, 1] and list(pp.debug_mis_counters()[:6]) == [1, 1, n, 0, n, 1]
    pp.apply(streams.random_stream(n, 1500, seed=1))
    src, dst = global_edges(partition_states(pp))
    _, _, want, want_mask, _, _ = model(src, dst, n, "random", 5)
    assert want.max() >= 3
    for col, mis, hh, m in ((L.pppcsr_colouring, L.pppcsr_mis, h, n), (L.ppcsr_colouring, L.ppcsr_mis, e.h, e.get_n())):
        assert col(hh, 0, 5, None, None, None) == EINVAL and mis(hh, 0, 5, None, None, None) == EINVAL
        assert col(None, 0, 5, colour.ctypes.data, ctypes.byref(ncol), None) == EINVAL
        assert mis(None, 0, 5, member.ctypes.data, ctypes.byref(size), None) == EINVAL
        for order in (3, 4, 0xFFFFFFFF):
            colour[:], member[:] = 77, 77
            assert col(hh, order, 5, colour.ctypes.data, ctypes.byref(ncol), None) == EINVAL
            assert mis(hh, order, 5, member.ctypes.data, ctypes.byref(size), None) == EINVAL
            assert np.all(colour == 77) and np.all(member == 77)
        ncol.value, size.value = 77, 1 << 40
        assert col(hh, 0, 5, None, ctypes.byref(ncol), None) == 0 and ncol.value != 77  # colour may be NULL, device_ms may be NULL
        assert mis(hh, 0, 5, None, ctypes.byref(size), None) == 0 and size.value <= m  # in_set may be NULL
        colour[:], member[:] = 77, 77
        assert col(hh, 0, 5, colour.ctypes.data, None, ctypes.byref(ms)) == 0 and ms.value >= 0.0  # ncolours may be NULL
        assert mis(hh, 0, 5, member.ctypes.data, None, ctypes.byref(ms)) == 0 and ms.value >= 0.0  # size may be NULL
        assert int(colour[:m].max()) + 1 == ncol.value and np.all(colour[m:] == 77)
        assert int(member[:m].sum()) == size.value and member[:m].max() == 1 and np.all(member[m:] == 77)
    assert L.pppcsr_colouring(h, 0, 5, colour.ctypes.data, ctypes.byref(ncol), None) == 0
    assert L.pppcsr_mis(h, 0, 5, member.ctypes.data, ctypes.byref(size), None) == 0
    np.testing.assert_array_equal(colour, want)
    np.testing.assert_array_equal(member.astype(bool), want_mask)
    assert L.ppcsr_debug_colouring_counters(None, colour.ctypes.data) == EINVAL and L.ppcsr_debug_colouring_counters(e.h, None) == EINVAL
    assert L.ppcsr_debug_mis_counters(None, colour.ctypes.data) == EINVAL and L.ppcsr_debug_mis_counters(e.h, None) == EINVAL
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_colouring(loc.h, 0, 5, colour.ctypes.data, ctypes.byref(ncol), None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_mis(loc.h, 0, 5, member.ctypes.data, ctypes.byref(size), None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one — tests/test_gpu_colouring.py)
    # the option: multiples of 64 in [64, 32768]
    for v in (64, 128, 4160, 32768):
        assert L.ppcsr_set_option(e.h, b"colour_window", v) == 0, v
    for v in (0, 1, 32, 63, 65, 96, 32767, 32769, 32832, 65536, -64, 1 << 40):
        assert L.ppcsr_set_option(e.h, b"colour_window", v) == EINVAL, v
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("what,order", [("colouring", "degree"), ("mis", "degree"), ("mis", "random")])
def test_sim_colouring_allocation_failures(lib, streams, what, order, P):
    """every device allocation of the call fails in turn: ENOMEM comes back, the state is unchanged, and the next call succeeds
    and equals the model"""
    def prepare(pp, states):
        n = pp.get_n()
        _, _, want, want_mask, _, _ = model(*global_edges(states), n, order, 3)
        colour, member = np.empty(n, np.uint32), np.empty(n, np.uint8)
        ncol, size = ctypes.c_uint32(), ctypes.c_uint64()

        def verify(k):
            if what == "colouring":
                got, top = pp.colouring(order, 3)
                np.testing.assert_array_equal(got, want)
                assert top == want.max() + 1
            else:
                got, count = pp.mis(order, 3)
                np.testing.assert_array_equal(got, want_mask)
                assert count == want_mask.sum()
        o = ORDERS.index(order)
        if what == "colouring":
            return lambda k: pp.L.pppcsr_colouring(pp.h, o, 3, colour.ctypes.data, ctypes.byref(ncol), None), lambda k: ENOMEM, verify
        return lambda k: pp.L.pppcsr_mis(pp.h, o, 3, member.ctypes.data, ctypes.byref(size), None), lambda k: ENOMEM, verify
    # colouring: the table, degrees, colours, cursors, pred, frontiers, keys, offsets, counters, the adjacency; mis: the
    # table, keys, states, marks, the blocked rounds, (degrees,) counters
    alloc_failures(lib, streams, P, prepare, 13 if what == "colouring" else 7 if order == "degree" else 6)
