"""CPU: ppcsr_triangles / ppcsr_common_neighbours and their pppcsr_ forms on the fiber SIMT emulator (tests/hostsim), which
compiles the engine's own kernel and host source.  Results are checked exactly against tests/triangles_model.py (wedge
enumeration over sorted keys, np.intersect1d over CSR rows, trace(A^3) / 6 for symmetric graphs), built from the exported
partition states."""
import ctypes

import numpy as np
import pytest

from consumers_model import global_edges, partition_states
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim
from test_sim_pppcsr_consumers import make, mixed_stream, tune
from triangles_model import assert_hard, hardness, model_common_neighbours, model_triangles, model_triangles_trace

EINVAL, EUNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


def pairs_for(pp, src, dst, extra=()):
    """pairs of every kind: stored edges, random pairs, a == b, repeats, vertices >= n, the seams between partitions"""
    n = pp.get_n()
    rng = np.random.default_rng(n)
    k = min(len(src), 150)
    pick = rng.choice(len(src), k, replace=False) if k else np.empty(0, np.int64)
    a = [src[pick], rng.integers(0, n, 150), np.arange(0, n, 97), np.array([n, 0, n + 7, 0xFFFFFFFF, 5, 5, 5])]
    b = [np.minimum(dst[pick], n + 3), rng.integers(0, n, 150), np.arange(0, n, 97), np.array([0, n, n, 3, 9, 9, 5])]
    P = pp.num_partitions()
    for q in range(1, P):  # the two vertices in different partitions
        f = int(pp.partition_start(q))
        if 0 < f < n:
            a.append(np.array([f - 1, f, 0]))
            b.append(np.array([f, f - 1, f]))
    for x, y in extra:
        a.append(np.array([x]))
        b.append(np.array([y]))
    return np.concatenate(a).astype(np.uint32), np.concatenate(b).astype(np.uint32)


def check(pp, label, hard=True, want_long=False, extra=()):
    """tri, total and common-neighbour counts against the model; nothing written (states and stats)"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    want_tri, want_total = model_triangles(src, dst, n)
    if hard:
        assert_hard(hardness(states, n, want_tri, want_total), label, want_long)
    tri, total = pp.triangles()
    assert total == want_total, (label, total, want_total)
    np.testing.assert_array_equal(tri, want_tri, err_msg=f"{label}: tri")
    none, total2 = pp.triangles(per_vertex=False)
    assert none is None and total2 == want_total, label
    a, b = pairs_for(pp, src, dst, extra)
    np.testing.assert_array_equal(pp.common_neighbours(a, b), model_common_neighbours(src, dst, n, a, b), err_msg=f"{label}: common")
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return want_tri, want_total


def dense_core(streams, n, count, seed):
    """folded RMAT adds, dense enough for thousands of triangles at n about 1200, with a self-loop"""
    s, d = streams.rmat_edges_folded(n, 11, count, seed=seed)
    return np.concatenate([streams.adds(s, d), np.array([[5, 5, 1]], np.uint32)])


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_triangles_model(lib, streams, P):
    """a bulk-built core under mixed streams (deletes, duplicate adds, destinations >= n), add_node twice and edges to the
    new vertices, a repartition to balanced_starts; then a bulk-built graph with a hub beyond the per-wave threshold"""
    n = 1200
    pp = make(lib, n, P)
    core = dense_core(streams, n, 30000, seed=60 + P)
    pp.bulk_build_device(core.ctypes.data, len(core))  # (emulator: device memory is host memory)
    ops = mixed_stream(streams, n, seed=40 + P)
    pp.apply(ops[: len(ops) // 2])
    pp.apply(ops[len(ops) // 2:])
    pp.apply(np.concatenate([core[:400:2, :2], np.zeros((200, 1), np.uint32)], axis=1))  # deletes of stored edges
    check(pp, f"P={P}")
    pp.add_node()
    pp.add_node()
    tail = [[n, 3, 2], [n, n + 1, 1], [7, n, 3], [7, n + 1, 3], [3, n, 1], [3, 7, 1], [3, n + 1, 1], [n + 5, 1, 1], [n + 1, n + 9, 1]]
    pp.apply(np.array(tail, np.uint32))
    tri, _ = check(pp, f"P={P} add_node")
    assert tri[n] >= 2 and tri[n + 1] >= 2  # (3, 7, n), (3, 7, n + 1), (3, n, n + 1), (7, n, n + 1)
    pp.repartition(pp.balanced_starts())
    tune(pp)
    check(pp, f"P={P} repartitioned")
    pp.close()

    hub = 3 if P == 1 else 2 * n // P + 1
    m = 5000
    rng = np.random.default_rng(P)
    leaf, hub2 = n - 2, hub + 2  # (hub, hub2): two long operands of comparable length
    adds = np.concatenate([streams.adds(np.full(m, hub, np.uint32), rng.permutation(m + 500)[:m].astype(np.uint32)),
                           streams.adds(np.full(m - 500, hub2, np.uint32), rng.permutation(m + 500)[:m - 500].astype(np.uint32)),
                           np.array([[hub, hub2, 1]], np.uint32),
                           streams.adds(np.arange(0, hub, 2, dtype=np.uint32), np.full((hub + 1) // 2, hub, np.uint32)),
                           np.array([[leaf, n - 1, 1], [hub, n + 40, 1], [hub, hub, 1]], np.uint32),
                           dense_core(streams, n, 30000, seed=9)])
    pp = make(lib, n, P)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    for v in (hub, hub2):
        node = pp.getNode(v)
        assert node[1] - node[0] > 4096
    extra = [(hub, hub), (hub, leaf), (leaf, hub), (hub, 0), (1, hub), (hub, hub2), (hub2, hub)]
    check(pp, f"P={P} hub", want_long=True, extra=extra)
    pp.apply(streams.random_stream(n, 500, seed=3, p_delete=0.3))
    check(pp, f"P={P} hub + stream", want_long=True, extra=extra)
    pp.close()


def test_sim_triangles_uniform_claims(lib, streams):
    """the same on a smaller graph with every wv::uni / wv::bcast of the kernels verified"""
    n = 500
    lib.ppcsr_sim_check_uniform(1)
    try:
        for P in (1, 3):
            pp = make(lib, n, P)
            core = dense_core(streams, n, 9000, seed=70)
            hubs = streams.adds(np.full(4500, 11, np.uint32), np.arange(4500, dtype=np.uint32))
            both = np.concatenate([core, hubs])
            pp.bulk_build_device(both.ctypes.data, len(both))
            check(pp, f"uniform P={P}", hard=False, extra=[(11, 11), (11, 12)])
            pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


def test_sim_triangles_symmetric_and_upper(lib, streams):
    """a graph stored symmetrically: the classical count trace(A^3) / 6; the upper-triangular copy of it: the same total"""
    n = 400
    s, d = streams.rmat_edges_folded(n, 9, 5000, seed=17)
    keep = s != d
    s, d = s[keep], d[keep]
    sym = streams.adds(np.concatenate([s, d]), np.concatenate([d, s]))
    up = streams.adds(np.minimum(s, d), np.maximum(s, d))
    totals = []
    for P, ops in ((1, sym), (3, sym), (1, up), (4, up)):
        pp = make(lib, n, P)
        pp.apply(ops)
        src, dst = global_edges(partition_states(pp))
        tri, total = pp.triangles()
        assert total == model_triangles(src, dst, n)[1]
        assert int(tri.sum()) == 3 * total
        totals.append(total)
        if ops is sym:
            assert total == model_triangles_trace(src, dst, n)
        pp.close()
    assert totals[0] > n and len(set(totals)) == 1, totals


def test_sim_triangles_zeros(lib, streams):
    """an empty graph; a graph without triangles (a bipartite one: low ids to high ids only, plus backward pairs)"""
    n = 300
    for P in (1, 3):
        pp = make(lib, n, P)
        tri, total = pp.triangles()
        assert total == 0 and not tri.any() and len(tri) == n
        assert not pp.common_neighbours([0, 5, n], [1, 5, 2]).any()
        rng = np.random.default_rng(P)
        lo, hi = rng.integers(0, n // 2, 2000), rng.integers(n // 2, n, 2000)
        ops = np.concatenate([streams.adds(lo.astype(np.uint32), hi.astype(np.uint32)), streams.adds(hi[:500].astype(np.uint32), lo[:500].astype(np.uint32))])
        pp.apply(ops)
        tri, total = pp.triangles()
        assert total == 0 and not tri.any()
        src, dst = global_edges(partition_states(pp))
        assert model_triangles(src, dst, n)[1] == 0
        a, b = pairs_for(pp, src, dst)
        got = pp.common_neighbours(a, b)
        np.testing.assert_array_equal(got, model_common_neighbours(src, dst, n, a, b))
        assert got.any()
        pp.close()


def test_sim_triangles_one_partition_is_the_engine(lib, streams):
    """P = 1: the results of ppcsr_triangles / ppcsr_common_neighbours[_device] on the partition's own engine; the staging
    seam of the host form moved into the batch"""
    n = 600
    pp = make(lib, n, 1)
    core = dense_core(streams, n, 12000, seed=4)
    pp.bulk_build_device(core.ctypes.data, len(core))
    e = pp.partition(0)
    tri, total = pp.triangles()
    tri_e, total_e, ms = e.triangles(with_ms=True)
    assert total_e == total and total > 0 and ms >= 0.0
    np.testing.assert_array_equal(tri, tri_e)
    assert e.triangles(per_vertex=False) == (None, total)
    src, dst = global_edges(partition_states(pp))
    a, b = pairs_for(pp, src, dst)
    want = model_common_neighbours(src, dst, n, a, b)
    np.testing.assert_array_equal(e.common_neighbours(a, b), want)
    out = np.zeros(len(a), np.uint32)
    e.common_neighbours_device(a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data)  # (emulator: device memory is host memory)
    np.testing.assert_array_equal(out, want)
    e.set_option("query_lookup_stage", 37)
    np.testing.assert_array_equal(e.common_neighbours(a, b), want)
    np.testing.assert_array_equal(pp.common_neighbours(a, b), want)
    assert len(e.common_neighbours([], [])) == 0
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_triangles_refuse_the_sequential_regime(lib, streams, P):
    """narrow == 0 on any partition: both calls return EUNSUPPORTED and say why, the state is intact and the engine usable;
    once a batch's range check has left the regime the results equal the model"""
    n = 500
    pp = make(lib, n, P)
    core = dense_core(streams, n, 8000, seed=23)
    pp.bulk_build_device(core.ctypes.data, len(core))
    states = partition_states(pp)
    e = pp.partition(P - 1)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    L = pp.L
    tri = np.full(n, 77, np.uint64)
    total = ctypes.c_uint64(77)
    a, b = np.array([1, 2], np.uint32), np.array([2, 3], np.uint32)
    cnt = np.full(2, 77, np.uint32)
    assert L.pppcsr_triangles(pp.h, tri.ctypes.data, ctypes.byref(total), None) == EUNSUPPORTED
    assert "sequential regime" in L.ppcsr_last_error().decode()
    assert L.pppcsr_common_neighbours(pp.h, a.ctypes.data, b.ctypes.data, 2, cnt.ctypes.data, None) == EUNSUPPORTED
    assert "sequential regime" in L.ppcsr_last_error().decode()
    assert L.ppcsr_triangles(e.h, tri.ctypes.data, ctypes.byref(total), None) == EUNSUPPORTED
    assert L.ppcsr_common_neighbours(e.h, a.ctypes.data, b.ctypes.data, 2, cnt.ctypes.data, None) == EUNSUPPORTED
    assert L.ppcsr_common_neighbours_device(e.h, a.ctypes.data, b.ctypes.data, 2, cnt.ctypes.data, None) == EUNSUPPORTED
    assert total.value == 77 and np.all(tri == 77) and np.all(cnt == 77)  # no number computed on a wrong assumption
    with pytest.raises(load_pkg().PpcsrError):
        pp.triangles()
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        np.testing.assert_array_equal(i0, i1)
        np.testing.assert_array_equal(n0, n1)
    pp.apply(streams.random_stream(n, 600, seed=5, p_delete=0.3))  # (routes ops to every partition: the range check runs)
    assert e.stats()["narrow"] == 1
    check(pp, f"P={P} after the regime", hard=False)
    pp.close()


def test_sim_triangles_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    pp.apply(streams.random_stream(n, 500, seed=1))
    L, h = pp.L, pp.h
    tri = np.empty(n, np.uint64)
    total = ctypes.c_uint64()
    ms = ctypes.c_double()
    a, b, cnt = np.zeros(4, np.uint32), np.ones(4, np.uint32), np.empty(4, np.uint32)
    A, B, C = a.ctypes.data, b.ctypes.data, cnt.ctypes.data
    e = pp.partition(0)
    for fn, hh in ((L.pppcsr_triangles, h), (L.ppcsr_triangles, e.h)):
        assert fn(hh, None, None, None) == EINVAL
        assert fn(None, tri.ctypes.data, ctypes.byref(total), None) == EINVAL
        assert fn(hh, tri.ctypes.data, None, None) == 0  # total may be NULL, device_ms may be NULL
        assert fn(hh, None, ctypes.byref(total), ctypes.byref(ms)) == 0 and ms.value >= 0.0
    for fn, hh in ((L.pppcsr_common_neighbours, h), (L.ppcsr_common_neighbours, e.h), (L.ppcsr_common_neighbours_device, e.h)):
        assert fn(None, A, B, 4, C, None) == EINVAL
        assert fn(hh, A, B, 4, None, None) == EINVAL
        assert fn(hh, None, B, 4, C, None) == EINVAL
        assert fn(hh, A, None, 4, C, None) == EINVAL
        assert fn(hh, None, None, 0, None, None) == 0  # k == 0: nothing to read or write
        assert fn(hh, A, B, 4, C, ctypes.byref(ms)) == 0 and ms.value >= 0.0
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_triangles(loc.h, tri.ctypes.data, ctypes.byref(total), None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_common_neighbours(loc.h, A, B, 4, C, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one — tests/test_gpu_triangles.py)
