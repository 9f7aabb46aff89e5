"""GPU: ppcsr_triangles / ppcsr_common_neighbours and their pppcsr_ forms on MI355X, all partitions on one device: against the
model of tests/triangles_model.py at RMAT scale 18 (wedge enumeration over sorted keys, np.intersect1d over CSR rows), 8
partitions against one PCSR at config #2's size, the device form on torch tensors, and a few rounds of batch-then-check at
scale 14."""
import ctypes

import numpy as np
import pytest

from consumers_model import global_edges, last_slot_free, partition_states
from helpers import load_pkg
from triangles_model import assert_hard, hardness, model_common_neighbours, model_triangles

pytestmark = pytest.mark.gpu


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


def pairs_for(pp, src, dst, k, extra=()):
    """stored edges, random pairs, a == b, repeats, vertices >= n, the seams between partitions, the busiest vertices"""
    n = pp.get_n()
    rng = np.random.default_rng(k)
    pick = rng.choice(len(src), k, replace=False)
    busy = np.argsort(np.bincount(src, minlength=n))[-8:]
    a = [src[pick], rng.integers(0, n, k), np.arange(0, n, 4099), np.array([n, 0, n + 7, 0xFFFFFFFF, 5, 5, 5]), busy, busy, busy]
    b = [np.minimum(dst[pick], n + 3), rng.integers(0, n, k), np.arange(0, n, 4099), np.array([0, n, n, 3, 9, 9, 5]), busy, busy[::-1],
         rng.integers(0, n, len(busy))]
    for q in range(1, pp.num_partitions()):
        f = int(pp.partition_start(q))
        if 0 < f < n:
            a.append(np.array([f - 1, f, 0]))
            b.append(np.array([f, f - 1, f]))
    for x, y in extra:
        a.append(np.array([x]))
        b.append(np.array([y]))
    return np.concatenate(a).astype(np.uint32), np.concatenate(b).astype(np.uint32)


def check_model(pp, label, want_long, pairs=2000, extra=(), hard=True):
    n = pp.get_n()
    states = partition_states(pp)
    src, dst = global_edges(states)
    want_tri, want_total = model_triangles(src, dst, n)
    h = hardness(states, n, want_tri, want_total)
    print(label, h, "largest tri", int(want_tri.max()))
    if hard:
        assert_hard(h, label, want_long)
    elif want_long:
        assert h["long"] >= 1, (label, h)
    tri, total = pp.triangles()
    print(label, "device total", total)
    assert total == want_total, (label, total, want_total)
    np.testing.assert_array_equal(tri, want_tri, err_msg=f"{label}: tri")
    assert pp.triangles(per_vertex=False) == (None, want_total), label
    a, b = pairs_for(pp, src, dst, pairs, extra)
    np.testing.assert_array_equal(pp.common_neighbours(a, b), model_common_neighbours(src, dst, n, a, b), err_msg=f"{label}: common")
    after = partition_states(pp)  # nothing written
    for (_, i0, n0), (_, i1, n1) in zip(states, after):
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1), label
    return want_tri, want_total


def test_triangles_model_rmat18(pkg, streams):
    """P = 8: a 2 M-edge RMAT core and a mixed stream, add_node, a repartition to balanced_starts; then a graph with a hub of
    2^20 edges (far beyond what a wave intersects on its own), bulk-built from a device tensor"""
    n, P = 1 << 18, 8
    s, d = streams.rmat_edges(18, 2_000_000, seed=31)
    core = streams.adds(s, d)
    s2, d2 = streams.rmat_edges(18, 300_000, seed=32)
    mixed = streams.mixed_existing_stream(core, streams.adds(s2, d2 + np.uint32(7)), seed=33)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    pp.apply(core)
    pp.apply(mixed)
    pp.add_node()
    pp.apply(np.array([[n, 1, 5], [2, n, 9], [1, n, 1], [1, 2, 1]], np.uint32))
    pp.add_node()  # (isolated)
    stats = [pp.partition(k).stats() for k in range(P)]
    tri, total = check_model(pp, "rmat18", want_long=True)
    assert stats == [pp.partition(k).stats() for k in range(P)]
    pp.repartition(pp.balanced_starts())
    check_model(pp, "rmat18 repartitioned", want_long=True)
    pp.close()

    m, nh = 1 << 20, 1 << 21
    hub = 3 * nh // 8 + 11
    rng = np.random.default_rng(5)
    s3, d3 = streams.rmat_edges_folded(nh, 21, 2_000_000, seed=34)
    adds = np.concatenate([streams.adds(s3, d3), streams.adds(np.full(m, hub, np.uint32), rng.permutation(nh)[:m].astype(np.uint32))])
    pp = pkg.PPPCSR(nh, numDomain=1, partitionsPerDomain=P)
    t = to_device(adds)
    pp.bulk_build_device(t.data_ptr(), len(adds))
    node = pp.getNode(hub)
    assert node[1] - node[0] > m
    # (one edge per vertex on average: this graph is here for the hub's range, and its triangles are those through the hub — the
    # long-operand condition is asserted, the density conditions belong to the graphs above)
    tri, total = check_model(pp, "hub", want_long=True, extra=[(hub, hub), (hub, 1), (hub - 1, hub)], hard=False)
    assert total > 0 and tri[hub] > 0


def test_triangles_match_one_engine_config2(pkg, streams):
    """config #2's graph (RMAT scale 20, 10 M core edges, bulk-built) and a 1 M mixed stream, on 8 partitions and on one
    PCSR: equal tri[], equal totals, equal common-neighbour counts for 1 M pairs; the device form equals the host form"""
    import torch
    n = 1 << 20
    s, d = streams.rmat_edges(20, 10_000_000, seed=1)
    core = streams.adds(s, d)
    s2, d2 = streams.rmat_edges(20, 1_000_000, seed=2)
    mixed = streams.mixed_existing_stream(core, streams.adds(s2, d2), seed=3)
    one = pkg.PCSR(n)
    one.bulk_build(core)
    one.apply(mixed)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    t = to_device(core)
    pp.bulk_build_device(t.data_ptr(), len(core))
    del t
    pp.apply(mixed)
    assert last_slot_free(one.state()[0])
    assert all(last_slot_free(i) for _, i, _ in partition_states(pp))
    ta, total_a = pp.triangles()
    tb, total_b = one.triangles()
    print("config2 triangles", total_a, "largest tri", int(ta.max()))
    np.testing.assert_array_equal(ta, tb)
    assert total_a == total_b and total_a > 0
    assert int(ta.sum()) == 3 * total_a
    assert pp.triangles(per_vertex=False) == (None, total_a) and one.triangles(per_vertex=False) == (None, total_a)
    k = 1_000_000
    rng = np.random.default_rng(9)
    pick = rng.choice(len(s), k // 2, replace=False)
    a = np.concatenate([s[pick], rng.integers(0, n + 5, k // 2)]).astype(np.uint32)
    b = np.concatenate([d[pick], rng.integers(0, n + 5, k // 2)]).astype(np.uint32)
    ca, cb = pp.common_neighbours(a, b), one.common_neighbours(a, b)
    np.testing.assert_array_equal(ca, cb)
    assert np.count_nonzero(ca) > k // 100 and int(ca.max()) > 64
    # the device form on torch tensors
    da, db = to_device(a), to_device(b)
    out = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    one.common_neighbours_device(da.data_ptr(), db.data_ptr(), k, out.data_ptr())
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), cb)


def test_common_neighbours_device_form(pkg, streams):
    """common_neighbours_device on torch tensors equals the host form and the model (scale 14), staged host form included"""
    import torch
    n = 1 << 14
    s, d = streams.rmat_edges(14, 120_000, seed=51)
    one = pkg.PCSR(n)
    one.apply(streams.adds(s, d))
    src, dst = global_edges([(0,) + tuple(one.state())])
    pp1 = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=1)
    a, b = pairs_for(pp1, src, dst, 3000)
    pp1.close()
    want = model_common_neighbours(src, dst, n, a, b)
    np.testing.assert_array_equal(one.common_neighbours(a, b), want)
    da, db = to_device(a), to_device(b)
    out = torch.full((len(a),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ms = one.common_neighbours_device(da.data_ptr(), db.data_ptr(), len(a), out.data_ptr(), with_ms=True)
    assert ms >= 0.0
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want)
    one.set_option("query_lookup_stage", 1000)
    np.testing.assert_array_equal(one.common_neighbours(a, b), want)
    tri, total = one.triangles()
    want_tri, want_total = model_triangles(src, dst, n)
    assert total == want_total and total > 100_000  # (150 582 for the raw stream)
    np.testing.assert_array_equal(tri, want_tri)


def test_triangles_follow_batches(pkg, streams):
    """3 rounds of: apply a batch, then triangles and common neighbours against the model (scale 14)"""
    n, P = 1 << 14, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges(14, 60_000, seed=61)
    pp.apply(streams.adds(s, d))
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 20_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 10_000, seed=80 + r, p_delete=0.5),
                                np.array([[r, r, 1], [r, n + r, 1]], np.uint32)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        check_model(pp, f"round {r}", want_long=False)


def test_triangles_status_codes(pkg, streams):
    """the sequential regime and partitions on two devices are refused with EUNSUPPORTED; argument errors with EINVAL"""
    n = 1 << 12
    s, d = streams.rmat_edges(12, 60_000, seed=41)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4)
    pp.apply(streams.adds(s, d))
    L = pp.L
    tri = np.empty(n, np.uint64)
    total = ctypes.c_uint64(77)
    assert L.pppcsr_triangles(pp.h, None, None, None) == 1
    assert L.pppcsr_triangles(None, tri.ctypes.data, None, None) == 1
    assert L.pppcsr_common_neighbours(pp.h, None, None, 3, None, None) == 1
    e = pp.partition(2)
    e.set_option("search_narrow", 0)
    assert L.pppcsr_triangles(pp.h, tri.ctypes.data, ctypes.byref(total), None) == 4 and total.value == 77
    assert "sequential regime" in L.ppcsr_last_error().decode()
    assert L.ppcsr_triangles(e.h, None, ctypes.byref(total), None) == 4 and total.value == 77
    e.set_option("search_narrow", 1)
    src, dst = global_edges(partition_states(pp))
    want_tri, want_total = model_triangles(src, dst, n)
    got, got_total = pp.triangles()
    assert got_total == want_total and want_total > 100_000  # (119 124 for the raw stream)
    np.testing.assert_array_equal(got, want_tri)
    if L.ppcsr_device_count() >= 2:
        two = pkg.PPPCSR(n, numDomain=2, partitionsPerDomain=1, devices=[0, 1])
        assert L.pppcsr_triangles(two.h, tri.ctypes.data, ctypes.byref(total), None) == 4
        assert "more than one device" in L.ppcsr_last_error().decode()
