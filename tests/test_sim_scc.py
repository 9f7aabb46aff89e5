"""CPU: ppcsr_scc / pppcsr_scc on the fiber SIMT emulator (tests/hostsim), which compiles the engine's own kernel and host
source.  Labels and counts are checked exactly against tests/scc_model.py (an iterative Tarjan on Python integers) built from
the exported partition states, and against closed forms; the counters of ppcsr_debug_scc_counters show that every phase of the
schedule does its own share (the phases cover for each other, so label parity alone cannot)."""
import ctypes

import numpy as np
import pytest

from consumers_model import global_edges, partition_states
from helpers import load_pkg
from scc_model import assert_hard, hardness, model_scc, trim_closure, zoo
from test_sim_engine import SIM_SO, build_sim
from test_sim_kcore import alloc_failures
from test_sim_pppcsr_consumers import make, mixed_stream, tune

EINVAL, EHIP = 1, 3
NO_PIVOT = 0xFFFFFFFFFFFFFFFF
ZOO = dict(n=1200, scale=11, core_edges=3000, cycles=12, longest=100, k=12, L=150)
ZOO_HARD = dict(nontrivial=20, distinct=10, largest=100, trim_sweeps=50, below=1, above=1, loops=4, beyond=1)


@pytest.fixture(scope="module")
def lib():
    build_sim()
    L = load_pkg().load_library(SIM_SO)
    L.ppcsr_sim_fail_alloc_after.argtypes = [ctypes.c_int]
    return L


def check(pp, label, **hard):
    """labels and count against the model, the conditions on the input from the model; nothing written (states and stats);
    returns (labels, hardness, counters, edges)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    want = model_scc(src, dst, n)
    h = hardness(src, dst, n, want)
    assert_hard(h, label, **hard)
    labels, count = pp.scc()
    np.testing.assert_array_equal(labels, want, err_msg=f"{label}: labels")
    assert count == int((want == np.arange(n)).sum()), (label, count)
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return want, h, pp.debug_scc_counters(), (src, dst)


def check_counters(c, want, src, dst, n, label):
    """every phase did its share: the three phases label every vertex once; the pivot's phase labelled exactly the pivot's SCC;
    trimming retired at least the trim closure of the whole graph"""
    assert int(c[0] + c[3] + c[5]) == n, (label, c)
    assert c[2] != NO_PIVOT and int(c[3]) == int((want == want[int(c[2])]).sum()), (label, c)
    assert int(c[0]) >= int(trim_closure(src, dst, n)[0].sum()), (label, c)
    assert c[1] >= 1 and c[6] >= c[1] and c[7] >= c[6], (label, c)


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_scc_zoo(lib, streams, P):
    """the zoo in two batches, a mixed stream with deletes, add_node three times and edges to and from the new vertices (one
    left isolated), a repartition to balanced_starts: labels, count and counters after each step.  P = 3 runs with every wv::uni /
    wv::bcast verified"""
    n = ZOO["n"]
    lib.ppcsr_sim_check_uniform(1 if P == 3 else 0)
    try:
        pp = make(lib, n, P)
        assert not pp.debug_scc_counters().any()  # all zeros before the first call
        ops = zoo(streams, seed=17, **ZOO)
        pp.apply(ops[: len(ops) // 2])
        pp.apply(ops[len(ops) // 2:])
        want, h, c, (src, dst) = check(pp, f"P={P}", **ZOO_HARD)
        check_counters(c, want, src, dst, n, f"P={P}")
        assert c[4] >= 1 and c[5] >= 1, c  # the colouring phase ran: the chain of two-cycles alone needs k rounds
        assert c[4] >= ZOO["k"], c
        comp = pp.components()
        for a, b in ((want, comp),):  # equal SCC label implies equal WCC label: both name a set by its smallest id
            np.testing.assert_array_equal(b[a], b)
            assert np.all(b <= a)
        pp.apply(mixed_stream(streams, n, seed=40 + P))
        want, h, c, (src, dst) = check(pp, f"P={P} mixed", beyond=1)
        check_counters(c, want, src, dst, n, f"P={P} mixed")
        pp.add_node()
        pp.add_node()
        pp.add_node()
        pp.apply(np.array([[n, 3, 2], [3, n, 1], [n, n + 1, 1], [n + 1, 7, 1], [n + 5, 1, 1], [n + 1, n + 9, 1]], np.uint32))
        want, h, c, (src, dst) = check(pp, f"P={P} add_node", beyond=1)
        check_counters(c, want, src, dst, n + 3, f"P={P} add_node")
        assert want[n] == want[3] and want[n + 2] == n + 2  # (n <-> 3: in 3's SCC; n + 2 is isolated)
        pp.repartition(pp.balanced_starts())
        tune(pp)
        want2, _, c, _ = check(pp, f"P={P} repartitioned")
        np.testing.assert_array_equal(want2, want)
        check_counters(c, want, src, dst, n + 3, f"P={P} repartitioned")
        pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


@pytest.mark.parametrize("P", [1, 4])
def test_sim_scc_rmat_needs_no_colouring(lib, streams, P):
    """a plain folded RMAT stream: one giant SCC and single vertices — trimming and one pivot suffice, and the pivot (the
    longest slot range) lies in the giant SCC"""
    n = ZOO["n"]
    pp = make(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 11, 6000, seed=41)
    pp.apply(streams.adds(s, d))
    want, h, c, (src, dst) = check(pp, f"rmat P={P}", largest=n // 8)
    assert h["nontrivial"] == 1, h
    check_counters(c, want, src, dst, n, f"rmat P={P}")
    assert c[4] == 0 and c[5] == 0, c
    assert int(c[3]) == h["largest"], (c, h)
    pp.close()


@pytest.mark.parametrize("P", [1, 4])
def test_sim_scc_closed_forms(lib, streams, P):
    """on permuted ids in one bulk-built stream: a complete digraph on 40 vertices, a directed cycle of 300, a directed path of
    300, a bidirectional path of 50 (one SCC), 20 isolated vertices; a vertex with 5000 out-edges and no in-edge, a vertex with
    5000 in-edges and no out-edge (5000 writers of one flag), and a hub with 5000 out-edges inside an SCC whose slot range is
    beyond what one wave walks"""
    n, m = 6000, 5000
    rng = np.random.default_rng(5 + P)
    perm = rng.permutation(n).astype(np.int64)
    parts = np.split(perm, np.cumsum([40, 300, 300, 50, 20, m, 1, 1, 2]))
    kq, cyc, path, bi, lone, leaves, (a,), (b,), (hub, back) = parts[:9]
    i, j = np.nonzero(~np.eye(40, dtype=bool))
    pairs = [np.stack([kq[i], kq[j]], axis=1), np.stack([cyc, np.roll(cyc, -1)], axis=1), np.stack([path[:-1], path[1:]], axis=1),
             np.stack([bi[:-1], bi[1:]], axis=1), np.stack([bi[1:], bi[:-1]], axis=1),
             np.stack([np.full(m, a), leaves], axis=1), np.stack([leaves, np.full(m, b)], axis=1),
             np.stack([np.full(m, hub), leaves], axis=1), np.array([[hub, back], [back, hub]])]
    rows = np.concatenate(pairs)
    ops = streams.adds(rows[:, 0].astype(np.uint32), rows[:, 1].astype(np.uint32))
    ops = ops[rng.permutation(len(ops))]
    want = np.arange(n, dtype=np.uint32)
    for group in (kq, cyc, bi, np.array([hub, back])):
        want[group] = group.min()
    pp = make(lib, n, P)
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    node = pp.getNode(int(hub))
    assert node[1] - node[0] > 4096
    labels, count = pp.scc()
    np.testing.assert_array_equal(labels, want)
    assert count == n - 39 - 299 - 49 - 1
    c = pp.debug_scc_counters()
    assert c[1] >= 150, c  # the path alone: two vertices per sweep
    _, h, _, _ = check(pp, f"closed P={P}", nontrivial=4, distinct=4, largest=300, trim_sweeps=150, max_out=m, max_in=m)
    pp.close()


def test_sim_scc_small_shapes(lib):
    """n = 0; n = 1 with and without a self-loop; vertices and no edge: every vertex an SCC of its own"""
    pkg = load_pkg()
    e = pkg.PCSR(0, lib=lib)
    labels, count = e.scc()
    assert len(labels) == 0 and count == 0
    assert e.debug_scc_counters()[2] == NO_PIVOT
    e = pkg.PCSR(1, lib=lib)
    assert [x.tolist() if hasattr(x, "tolist") else x for x in e.scc()] == [[0], 1]
    e.add_edge(0, 0, 1)
    labels, count = e.scc()
    assert labels.tolist() == [0] and count == 1
    for P in (1, 3):
        pp = make(lib, 300, P)
        labels, count = pp.scc()
        np.testing.assert_array_equal(labels, np.arange(300))
        assert count == 300
        c = pp.debug_scc_counters()
        assert c[0] == 300 and c[1] == 1 and c[2] == NO_PIVOT and not c[3:6].any(), c
        pp.close()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_scc_answers_in_the_sequential_regime(lib, streams, P):
    """narrow == 0 on one partition: the call is not refused (it intersects nothing) and equals the model"""
    n = 500
    pp = make(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 9, 3000, seed=23)
    adds = streams.adds(s, d)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    e = pp.partition(P - 1)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    tri = np.empty(n, np.uint64)
    assert pp.L.pppcsr_triangles(pp.h, tri.ctypes.data, None, None) == 4  # (the regime is the one triangles refuses)
    check(pp, f"sequential P={P}", largest=50)
    labels, _ = e.scc()
    assert len(labels) == e.get_n()
    assert e.stats()["narrow"] == 0
    pp.close()


def test_sim_scc_errors(lib, streams):
    n = 300
    pp = make(lib, n, 3)
    L, h = pp.L, pp.h
    e = pp.partition(0)
    pp.apply(streams.random_stream(n, 900, seed=1))
    want = model_scc(*global_edges(partition_states(pp)), n)
    labels = np.full(n, 77, np.uint32)
    count = ctypes.c_uint64(77)
    ms = ctypes.c_double()
    out = np.zeros(8, np.uint64)
    for fn, hh, m in ((L.pppcsr_scc, h, n), (L.ppcsr_scc, e.h, e.get_n())):
        assert fn(hh, None, None, None) == EINVAL
        assert fn(None, labels.ctypes.data, ctypes.byref(count), None) == EINVAL
        count.value = 77
        assert fn(hh, None, ctypes.byref(count), None) == 0 and count.value != 77  # labels may be NULL, device_ms may be NULL
        total = count.value
        labels[:] = 77
        assert fn(hh, labels.ctypes.data, None, ctypes.byref(ms)) == 0 and ms.value >= 0.0  # count may be NULL
        assert int((labels[:m] == np.arange(m)).sum()) == total and np.all(labels[m:] == 77)
    assert L.pppcsr_scc(h, labels.ctypes.data, ctypes.byref(count), None) == 0
    np.testing.assert_array_equal(labels, want)
    assert L.ppcsr_debug_scc_counters(None, out.ctypes.data) == EINVAL
    assert L.ppcsr_debug_scc_counters(e.h, None) == EINVAL
    assert L.ppcsr_debug_scc_counters(e.h, out.ctypes.data) == 0 and int(out[0] + out[3] + out[5]) == n
    # a handle that holds only some partitions of its layout
    loc = load_pkg().PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_scc(loc.h, labels.ctypes.data, ctypes.byref(count), None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    pp.close()


def test_sim_scc_allocation_failures(lib, streams):
    """every device allocation of the call fails in turn: the allocation status comes back, the state is unchanged, and the
    next call succeeds and equals the model"""
    def prepare(pp, states):
        n = pp.get_n()
        want = model_scc(*global_edges(states), n)
        labels = np.empty(n, np.uint32)
        count = ctypes.c_uint64()

        def verify(k):
            got, total = pp.scc()
            np.testing.assert_array_equal(got, want)
            assert total == int((want == np.arange(n)).sum())
        return lambda k: pp.L.pppcsr_scc(pp.h, labels.ctypes.data, ctypes.byref(count), None), lambda k: EHIP, verify
    for P in (1, 3):
        # the table, labels, colours, the live bitmap, two flag arrays, two mark arrays, the counters, the pivot's words
        alloc_failures(lib, streams, P, prepare, 10)


def test_scc_model_against_scipy_and_networkx(streams):
    """the model itself against scipy's and networkx's strong components, on the zoo"""
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    nx = pytest.importorskip("networkx")
    n = ZOO["n"]
    ops = zoo(streams, seed=17, **ZOO)
    src, dst = ops[:, 0].astype(np.int64), ops[:, 1].astype(np.int64)
    want = model_scc(src, dst, n)
    assert_hard(hardness(src, dst, n, want), "zoo", **ZOO_HARD)
    ok = dst < n
    ncomp, lab = csgraph.connected_components(sp.csr_matrix((np.ones(int(ok.sum())), (src[ok], dst[ok])), shape=(n, n)), connection="strong")
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    np.testing.assert_array_equal(want, smallest[lab])
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(src[ok].tolist(), dst[ok].tolist()))
    ref = np.empty(n, np.int64)
    for comp in nx.strongly_connected_components(g):
        ref[list(comp)] = min(comp)
    np.testing.assert_array_equal(want, ref)
