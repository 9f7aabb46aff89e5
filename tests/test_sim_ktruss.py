"""CPU: ppcsr_edge_support / ppcsr_ktruss on the fiber SIMT emulator (tests/hostsim), which compiles the engine's own kernel and
host source.  Results are checked exactly against tests/truss_model.py (a synchronous sub-round peel over the triangle list, built
from the exported partition states) and against closed forms; the graphs and checks are those of tests/test_gpu_ktruss.py
(tests/truss_checks.py), at emulator sizes."""
import ctypes

import numpy as np
import pytest

import isect_graphs
import truss_checks as tc
from consumers_model import last_slot_free, partition_states
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim
from test_sim_kcore import alloc_failures
from test_sim_pppcsr_consumers import make, mixed_stream, tune
from truss_model import model_truss, rows_of


@pytest.fixture(scope="module")
def lib():
    build_sim()
    L = load_pkg().load_library(SIM_SO)
    L.ppcsr_sim_fail_alloc_after.argtypes = [ctypes.c_int]
    return L


@pytest.mark.parametrize("P", [1, 3])
def test_sim_ktruss_closed_forms(lib, P):
    tc.check_k9(lambda n: make(lib, n, P))
    tc.check_closed_forms(lambda n: make(lib, n, P), seed=3 + P)


@pytest.mark.parametrize("P", [1, 4])
def test_sim_ktruss_cylinder(lib, P):
    tc.check_cylinder(lambda n: make(lib, n, P))


@pytest.mark.parametrize("P", [1, 3])
def test_sim_ktruss_book(lib, P):
    tc.check_book(lambda n: make(lib, n, P))


def rmat_graph(lib, streams, n, P):
    """a bulk-built folded RMAT core under tc.rmat_stream's mixed stream (deletes, duplicate adds, destinations >= n, a planted
    K_32) and the consumers' own mixed stream, add_node twice and edges to and from the new vertices"""
    pp = make(lib, n, P)
    core, mixed = tc.rmat_stream(streams, n, 11, 9000, seed=41, folded=True)
    pp.bulk_build_device(core.ctypes.data, len(core))  # (emulator: device memory is host memory)
    pp.apply(mixed)
    pp.apply(mixed_stream(streams, n, seed=40))
    pp.add_node()
    pp.add_node()
    pp.apply(np.array([[n, 3, 2], [7, n, 3], [3, n, 1], [9, n, 1], [3, 7, 1], [3, 9, 1], [7, 9, 1], [n, n + 1, 1], [n + 5, 1, 1], [n + 1, n + 9, 1]], np.uint32))
    return pp


def test_sim_ktruss_rmat_across_partitions(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and a repartition that leaves an empty partition: outputs equal word for word; P = 1 equals
    the partition's own engine call.  P = 4 runs with every wv::uni / wv::bcast claim verified"""
    n = 1200
    hard = dict(tmax=20, distinct=6, gaps=10, levels=6, max_subrounds=3, below_support=n // 8, max_support=40, first_frontier=1000,
                backward=1, loops=1, beyond=1)
    results = []
    for P in (1, 2, 4, 8):
        lib.ppcsr_sim_check_uniform(1 if P == 4 else 0)
        try:
            pp = rmat_graph(lib, streams, n, P)
            assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
            mt, h, _ = tc.check(pp, f"P={P}", identities=P in (1, 4), **hard, **({"cross": 100} if P > 1 else {}))
            assert mt["truss"][(mt["a"] == 3) & (mt["b"] == n)][0] >= 4  # (n with 3, 7, 9: a K4 through the new vertex)
            results.append((pp.edge_support(), pp.ktruss()))
            if P == 1:
                e = pp.partition(0)
                tc.same(e.edge_support(), results[0][0])
                tc.same(e.ktruss(), results[0][1])
                np.testing.assert_array_equal(e.debug_ktruss_counters()[:7], pp.debug_ktruss_counters()[:7])
            if P == 4:
                pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
                tune(pp)
                tc.check(pp, "P=4 repartitioned", identities=False, **hard)
                results.append((pp.edge_support(), pp.ktruss()))
            pp.close()
        finally:
            lib.ppcsr_sim_check_uniform(0)
    for sup, tr in results[1:]:
        tc.same(sup, results[0][0])
        tc.same(tr, results[0][1])


@pytest.mark.parametrize("P", [1, 3])
def test_sim_ktruss_constructed_hubs(lib, streams, P):
    """tests/isect_graphs.py's 4000-vertex graph: 16 hubs beyond 4096 + 64 slots, their edges deferred in the support phase and
    in the peel, ranges full of destinations >= n behind the counted ones"""
    pp = isect_graphs.build(load_pkg(), lib, streams, P, emulator=True)
    for hub in pp.isect_hubs:
        node = pp.getNode(hub)
        assert node[1] - node[0] - 1 > tc.WAVE_SLOTS + 64
    _, _, ctr = tc.check(pp, f"hubs P={P}", identities=P == 1, tmax=6, distinct=5, beyond=10000, loops=1, below_support=1000, max_subrounds=3)
    assert ctr[6] >= 1, ctr
    pp.close()


def test_sim_ktruss_follow_batches(lib, streams):
    """3 rounds of: apply a batch of adds, deletes, a self-loop and a destination >= n, then both calls against the model"""
    n, P = 600, 3
    pp = make(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 10, 4000, seed=61)
    pp.apply(streams.adds(s, d))
    for r in range(3):
        s2, d2 = streams.rmat_edges_folded(n, 10, 1500, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 800, seed=80 + r, p_delete=0.5),
                                np.array([[r, r, 1], [r, n + r, 1]], np.uint32)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        tc.check(pp, f"round {r}", identities=r == 2, tmax=5, distinct=4, backward=1, loops=1, beyond=1)
    pp.close()


def test_sim_ktruss_status_codes(lib, streams):
    pp = tc.check_status_codes(load_pkg(), lambda n, P: make(lib, n, P), streams, 300, lib=lib)
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one — tests/test_gpu_ktruss.py)
    pp.close()
    # n = 0
    e = load_pkg().PCSR(0, lib=lib)
    edges, total = e.edge_support()
    assert edges.shape == (0, 3) and total == 0
    edges, tmax, vtruss = e.ktruss()
    assert edges.shape == (0, 3) and tmax == 0 and len(vtruss) == 0
    count = ctypes.c_uint64(7)
    assert lib.ppcsr_ktruss(e.h, None, 0, ctypes.byref(count), None, None, None) == 0 and count.value == 0


def test_sim_ktruss_counters_start_at_zero(lib):
    e = load_pkg().PCSR(10, lib=lib)
    assert not e.debug_ktruss_counters().any()


@pytest.mark.parametrize("name", ["ktruss", "edge_support"])
def test_sim_ktruss_allocation_failures(lib, streams, name):
    """every device allocation of the call fails in turn: ENOMEM comes back, the state is unchanged, nothing leaks into the next
    call, which succeeds and equals the model"""
    def prepare(pp, states):
        _, _, _, mt, _ = tc.model_of(pp)
        m = len(mt["a"])
        buf = np.empty((m, 3), np.uint32)
        vt = np.empty(pp.get_n(), np.uint32)
        count, total, tmax = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        if name == "ktruss":
            call = lambda k: pp.L.pppcsr_ktruss(pp.h, buf.ctypes.data, m, ctypes.byref(count), ctypes.byref(tmax), vt.ctypes.data, None)
            verify = lambda k: tc.same(pp.ktruss(), (rows_of(mt["a"], mt["b"], mt["truss"]), mt["tmax"], mt["vtruss"]))
        else:
            call = lambda k: pp.L.pppcsr_edge_support(pp.h, buf.ctypes.data, m, ctypes.byref(count), ctypes.byref(total), None)
            verify = lambda k: tc.same(pp.edge_support(), (rows_of(mt["a"], mt["b"], mt["support"]), mt["total"]))
        return call, lambda k: tc.ENOMEM, verify
    for P in (1, 3):
        # the table; stamps, supports, (truss numbers), in-degrees, cursors, chunk counts, two offset arrays, tile sums, (vtruss),
        # the triangle total, counters; the in-lists (two), the deferred list, (two frontiers), the output
        alloc_failures(lib, streams, P, prepare, 19 if name == "ktruss" else 15)


def test_sim_ktruss_slot_search(lib):
    tc.check_slot_search(load_pkg().PCSR(8, lib=lib))
