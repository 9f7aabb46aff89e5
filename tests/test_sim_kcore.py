"""CPU: ppcsr_kcore / pppcsr_kcore on the fiber SIMT emulator (tests/hostsim), which compiles the engine's own kernel and host
source.  Results are checked exactly against tests/kcore_model.py (Batagelj-Zaversnik bucket peeling on Python integers, and a
synchronous numpy peel beside it), built from the exported partition states, and against closed forms."""
import ctypes

import numpy as np
import pytest

from consumers_model import global_edges, last_slot_free, model_bfs, partition_states
from helpers import load_pkg
from kcore_model import assert_hard, hardness, model_kcore
from paths_model import global_edges_valued, model_components, model_sssp
from test_sim_engine import SIM_SO, build_sim
from test_sim_pppcsr_consumers import make, mixed_stream, tune
from triangles_model import model_common_neighbours, model_triangles

EINVAL, ENOMEM, EHIP, EUNSUPPORTED = 1, 2, 3, 4


@pytest.fixture(scope="module")
def lib():
    build_sim()
    L = load_pkg().load_library(SIM_SO)
    L.ppcsr_sim_fail_alloc_after.argtypes = [ctypes.c_int]
    return L


def check(pp, label, **hard):
    """core and kmax against the model, the conditions on the input from the model; nothing written (states and stats)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    want = model_kcore(src, dst, n)
    h = hardness(src, dst, n, want)
    assert_hard(h, label, **hard)
    core, kmax = pp.kcore()
    np.testing.assert_array_equal(core, want, err_msg=f"{label}: core")
    assert kmax == h["kmax"] == (int(want.max()) if n else 0), (label, kmax, h)
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return want, h


def upper(pairs):
    """rows (min, max, 1) of undirected pairs"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.stack([p.min(axis=1), p.max(axis=1), np.ones(len(p), np.int64)], axis=1).astype(np.uint32)


def clique(ids):
    ids = np.asarray(ids)
    i, j = np.triu_indices(len(ids), 1)
    return np.stack([ids[i], ids[j]], axis=1)


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_kcore_model(lib, streams, P):
    """a bulk-built folded RMAT core under a mixed stream (deletes, duplicate adds, destinations >= n), add_node twice and
    edges to and from the new vertices, a repartition to balanced_starts.  P = 3 runs with every wv::uni / wv::bcast verified"""
    n = 1200
    hard = dict(kmax=8, distinct=8, max_subrounds=3, below_degree=n // 8, isolated=1, backward=1, loops=1, beyond=1)
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
        core, _ = check(pp, f"P={P} add_node", **hard)
        assert core[n] >= 2 and core[n + 1] >= 1  # (n: neighbours 3, 7, 9 in the dense part; stored dests n, n + 1 count now)
        pp.repartition(pp.balanced_starts())
        tune(pp)
        check(pp, f"P={P} repartitioned", **hard)
        pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


@pytest.mark.parametrize("P", [1, 4])
def test_sim_kcore_closed_forms(lib, P):
    """a clique K_30 (core 29), a cycle (2), a tree (1) and isolated vertices (0) on permuted ids in one shuffled stream: the
    levels 3 .. 28 exist for no vertex and are skipped; then the orientation convention"""
    n = 400
    rng = np.random.default_rng(3 + P)
    perm = rng.permutation(n)
    kq, cyc, tree, lone = perm[:30], perm[30:80], perm[80:200], perm[200:]
    pairs = [clique(kq), np.stack([cyc, np.roll(cyc, -1)], axis=1),
             np.array([[tree[i], tree[rng.integers(0, i)]] for i in range(1, len(tree))])]
    ops = upper(np.concatenate(pairs))
    ops = ops[rng.permutation(len(ops))]
    want = np.zeros(n, np.uint32)
    want[kq], want[cyc], want[tree] = 29, 2, 1
    pp = make(lib, n, P)
    pp.apply(ops)
    core, kmax = pp.kcore()
    np.testing.assert_array_equal(core, want)
    assert kmax == 29 and not core[lone].any()
    _, h = check(pp, f"closed P={P}", gaps=26, isolated=len(lone))
    assert h["distinct"] == 4
    # a self-loop, a destination >= n and backward pairs (between isolated vertices, and inside the tree) change nothing
    a, b = sorted(int(x) for x in lone[:2])
    pp.apply(np.array([[a, a, 1], [a, n + 3, 1], [b, a, 1], [max(tree[0], tree[5]), min(tree[0], tree[5]), 1]], np.uint32))
    core2, kmax2 = pp.kcore()
    np.testing.assert_array_equal(core2, want)
    assert core2[a] == 0 and core2[b] == 0 and kmax2 == 29  # only (b, a), b > a, stored: core 0 at both ends
    check(pp, f"closed P={P} + no-ops", backward=2, loops=1, beyond=1)
    # both directions stored: the same cores as the upper triangle alone
    pp.apply(ops[:, [1, 0, 2]])
    core3, kmax3 = pp.kcore()
    np.testing.assert_array_equal(core3, want)
    assert kmax3 == 29
    pp.close()


@pytest.mark.parametrize("P", [1, 4])
def test_sim_kcore_many_subrounds(lib, P):
    """a path over 600 permuted vertices: core 1 everywhere, after 300 sub-rounds of two vertices each; 40 disjoint cycles
    beside it, core 2"""
    n, L = 1000, 600
    rng = np.random.default_rng(12)
    perm = rng.permutation(n)
    path, rest = perm[:L], perm[L:]
    cycles = rest.reshape(40, 10)
    pairs = [np.stack([path[:-1], path[1:]], axis=1)] + [np.stack([c, np.roll(c, -1)], axis=1) for c in cycles]
    ops = upper(np.concatenate(pairs))
    pp = make(lib, n, P)
    pp.apply(ops[rng.permutation(len(ops))])
    want = np.zeros(n, np.uint32)
    want[path], want[rest] = 1, 2
    core, kmax = pp.kcore()
    np.testing.assert_array_equal(core, want)
    assert kmax == 2
    _, h = check(pp, f"path P={P}", max_subrounds=300)
    assert h["max_subrounds"] == 300 and h["levels"] == 2
    pp.close()


@pytest.mark.parametrize("P,hub", [(1, 7), (3, 5990)])
def test_sim_kcore_hub_and_long_list(lib, streams, P, hub):
    """a hub with 5000 leaves — 5000 decrements of one counter in one sub-round, and a list beyond what one wave walks, left
    to the second launch — that is also adjacent to 60 members of a clique K_100: leaves 1, hub 60, clique 99.  The hub with
    a small id is the source of its stored pairs (runs that fill waves), with a large id the destination of nearly all"""
    n = 6000
    rng = np.random.default_rng(P)
    others = rng.permutation(np.setdiff1d(np.arange(n), [hub]))
    leaves, kq = others[:5000], others[5000:5100]
    pairs = np.concatenate([np.stack([np.full(5000, hub), leaves], axis=1), clique(kq), np.stack([np.full(60, hub), kq[:60]], axis=1)])
    ops = upper(pairs)
    ops = ops[rng.permutation(len(ops))]
    pp = make(lib, n, P)
    pp.bulk_build_device(ops.ctypes.data, len(ops))  # (emulator: device memory is host memory)
    want = np.zeros(n, np.uint32)
    want[leaves], want[hub], want[kq] = 1, 60, 99
    core, kmax = pp.kcore()
    np.testing.assert_array_equal(core, want)
    assert kmax == 99
    _, h = check(pp, f"hub P={P}", maxdeg=4097, widest=5000, gaps=90)
    assert h["maxdeg"] == 5060
    pp.close()


def test_sim_kcore_invariant(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and one graph before and after a repartition with an empty partition: equal results;
    P = 1 equals the partition's own engine call"""
    n = 1000
    s, d = streams.rmat_edges_folded(n, 10, 5000, seed=6)
    adds, ops = streams.adds(s, d), mixed_stream(streams, n, seed=5)
    results = []
    for P in (1, 2, 4, 8):
        pp = make(lib, n, P)
        pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
        pp.apply(ops)
        assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
        results.append(pp.kcore())
        if P == 1:
            core, kmax, ms = pp.partition(0).kcore(with_ms=True)
            np.testing.assert_array_equal(core, results[0][0])
            assert kmax == results[0][1] and ms >= 0.0
            check(pp, "invariant", kmax=4, distinct=5)
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
            tune(pp)
            assert all(last_slot_free(i) for _, i, _ in partition_states(pp))
            results.append(pp.kcore())
        pp.close()
    for core, kmax in results[1:]:
        np.testing.assert_array_equal(core, results[0][0])
        assert kmax == results[0][1]


@pytest.mark.parametrize("P", [1, 3])
def test_sim_kcore_answers_in_the_sequential_regime(lib, streams, P):
    """narrow == 0 on one partition: the call is not refused (it intersects nothing) and equals the model"""
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
    check(pp, f"sequential P={P}", kmax=4)
    core, kmax = e.kcore()
    assert len(core) == e.get_n()
    assert e.stats()["narrow"] == 0
    pp.close()


def test_sim_kcore_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    L, h = pp.L, pp.h
    e = pp.partition(0)
    core = np.full(n, 77, np.uint32)
    kmax = ctypes.c_uint32(77)
    ms = ctypes.c_double()
    # n vertices and no edge: all zeros, kmax 0
    assert L.pppcsr_kcore(h, core.ctypes.data, ctypes.byref(kmax), None) == 0
    assert not core.any() and kmax.value == 0
    got, top = e.kcore()
    assert len(got) == e.get_n() and not got.any() and top == 0
    pp.apply(streams.random_stream(n, 1500, seed=1))
    src, dst = global_edges(partition_states(pp))
    want = model_kcore(src, dst, n)
    assert want.max() >= 2
    for fn, hh, m in ((L.pppcsr_kcore, h, n), (L.ppcsr_kcore, e.h, e.get_n())):
        assert fn(hh, None, None, None) == EINVAL
        assert fn(None, core.ctypes.data, ctypes.byref(kmax), None) == EINVAL
        kmax.value = 77
        assert fn(hh, None, ctypes.byref(kmax), None) == 0 and kmax.value != 77  # core may be NULL, device_ms may be NULL
        top = kmax.value
        core[:] = 77
        assert fn(hh, core.ctypes.data, None, ctypes.byref(ms)) == 0 and ms.value >= 0.0  # kmax may be NULL
        assert int(core[:m].max()) == top and np.all(core[m:] == 77)
    assert L.pppcsr_kcore(h, core.ctypes.data, ctypes.byref(kmax), None) == 0
    np.testing.assert_array_equal(core, want)
    assert kmax.value == want.max()
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_kcore(loc.h, core.ctypes.data, ctypes.byref(kmax), None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one — tests/test_gpu_kcore.py)
    pp.close()


def alloc_failures(lib, streams, P, prepare, min_allocs):
    """Every device allocation of one consumer call fails in turn.  prepare(pp, states) -> (call, expect, verify): call(k) is
    the C call whose k-th allocation fails (k = 0: none does) and returns its status, expect(k) is the status that failure
    must give, verify(k) runs the next call and compares it with the model.  After each failure the partition states are
    unchanged."""
    n = 400
    counter = ctypes.c_int.in_dll(lib, "g_sim_fail_alloc")
    pp = make(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 9, 3000, seed=8)
    pp.apply(streams.adds(s, d))
    states = partition_states(pp)
    call, expect, verify = prepare(pp, states)
    counter.value = 1 << 30
    assert call(0) == 0
    allocs = (1 << 30) - counter.value
    lib.ppcsr_sim_fail_alloc_after(0)
    assert allocs >= min_allocs, allocs
    for k in range(1, allocs + 1):
        lib.ppcsr_sim_fail_alloc_after(k)
        try:
            rc = call(k)
        finally:
            lib.ppcsr_sim_fail_alloc_after(0)
        assert rc == expect(k), (k, rc)
        for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
            np.testing.assert_array_equal(i0, i1)
            np.testing.assert_array_equal(n0, n1)
        verify(k)
    pp.close()


def test_sim_kcore_allocation_failures(lib, streams):
    """every device allocation of the call fails in turn: the allocation status comes back, the state is unchanged, and the
    next call succeeds and equals the model"""
    def prepare(pp, states):
        n = pp.get_n()
        want = model_kcore(*global_edges(states), n)
        core = np.empty(n, np.uint32)
        kmax = ctypes.c_uint32()

        def verify(k):
            got, top = pp.kcore()
            np.testing.assert_array_equal(got, want)
            assert top == want.max()
        # (EHIP: what a failed allocation of bfs / sssp / components returns)
        return lambda k: pp.L.pppcsr_kcore(pp.h, core.ctypes.data, ctypes.byref(kmax), None), lambda k: EHIP, verify
    for P in (1, 3):
        # the table, degrees, cores, offsets, cursors, frontiers, counters, the adjacency
        alloc_failures(lib, streams, P, prepare, 8)


def _prepare_bfs(pp, states):
    n, start = pp.get_n(), 3
    want, _ = model_bfs(*global_edges(states), n, start)
    out = np.empty(n, np.uint32)
    return (lambda k: pp.L.pppcsr_bfs(pp.h, start, out.ctypes.data, None), lambda k: EHIP,
            lambda k: np.testing.assert_array_equal(pp.bfs(start), want))


def _prepare_sssp(pp, states):
    n, start = pp.get_n(), 3
    want = model_sssp(*global_edges_valued(states), n, start)
    out = np.empty(n, np.uint64)
    return (lambda k: pp.L.pppcsr_sssp(pp.h, start, out.ctypes.data, None), lambda k: EHIP,
            lambda k: np.testing.assert_array_equal(pp.sssp(start), want))


def _prepare_components(pp, states):
    n = pp.get_n()
    want = model_components(*global_edges(states), n)
    out = np.empty(n, np.uint32)
    return (lambda k: pp.L.pppcsr_components(pp.h, out.ctypes.data, None), lambda k: EHIP,
            lambda k: np.testing.assert_array_equal(pp.components(), want))


def _prepare_triangles(pp, states):
    n = pp.get_n()
    want, total = model_triangles(*global_edges(states), n)
    tri = np.empty(n, np.uint64)
    tot = ctypes.c_uint64()

    def verify(k):
        got, t = pp.triangles()
        np.testing.assert_array_equal(got, want)
        assert t == total
    return lambda k: pp.L.pppcsr_triangles(pp.h, tri.ctypes.data, ctypes.byref(tot), None), lambda k: EHIP, verify


def _prepare_common_neighbours(pp, states):
    """the host form stages the pairs in three buffers that grow with the batch and are kept: every call brings a longer batch
    than any before it, so that each call allocates the table and the three of them"""
    n = pp.get_n()
    src, dst = global_edges(states)
    rng = np.random.default_rng(5)

    def pairs(m):
        return rng.integers(0, n + 20, m).astype(np.uint32), rng.integers(0, n + 20, m).astype(np.uint32)

    def call(k):
        a, b = pairs(128 * (k + 1))
        out = np.empty(len(a), np.uint32)
        return pp.L.pppcsr_common_neighbours(pp.h, a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data, None)

    def verify(k):
        a, b = pairs(128 * (k + 1) + 64)
        np.testing.assert_array_equal(pp.common_neighbours(a, b), model_common_neighbours(src, dst, n, a, b))
    # the table is a device allocation of the call (EHIP); the staging buffers report out of memory (ENOMEM)
    return call, lambda k: EHIP if k == 1 else ENOMEM, verify


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("prepare,min_allocs", [(_prepare_bfs, 7), (_prepare_sssp, 8), (_prepare_components, 3), (_prepare_triangles, 5),
                                                (_prepare_common_neighbours, 4)],
                         ids=["bfs", "sssp", "components", "triangles", "common_neighbours"])
def test_sim_consumer_allocation_failures(lib, streams, prepare, min_allocs, P):
    """the allocation path of every consumer that takes its buffers from the device per call, as
    test_sim_kcore_allocation_failures: each allocation fails in turn, the status is the allocation's, nothing is written,
    and the next call equals the model.  (pagerank is not among them: its first call allocates scratch that the partitions keep, so
    later calls make fewer allocations than the counted one and this helper fails on it — before the consumers shared one
    allocation path just as after.)"""
    alloc_failures(lib, streams, P, prepare, min_allocs)


def test_kcore_model_against_networkx(lib, streams):
    """the model itself against networkx.core_number on the symmetrised upper graph"""
    nx = pytest.importorskip("networkx")
    from triangles_model import upper_edges
    n = 700
    pp = make(lib, n, 3)
    s, d = streams.rmat_edges_folded(n, 10, 6000, seed=14)
    adds = streams.adds(s, d)
    pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
    pp.apply(mixed_stream(streams, n, seed=8))
    src, dst = global_edges(partition_states(pp))
    a, b = upper_edges(src, dst, n)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(a.tolist(), b.tolist()))
    ref = nx.core_number(g)
    want = model_kcore(src, dst, n)
    np.testing.assert_array_equal(want, np.array([ref[v] for v in range(n)], np.uint32))
    h = hardness(src, dst, n, want)
    assert h["kmax"] >= 6 and h["distinct"] >= 6, h
    np.testing.assert_array_equal(pp.kcore()[0], want)
    pp.close()
