"""GPU: ppcsr_sssp / ppcsr_components and their pppcsr_ forms on MI355X, all partitions on one device: against the model of
tests/paths_model.py at RMAT scale 18 (heap Dijkstra on Python integers, union-find), 8 partitions against one PCSR at config
#2's size, distances beyond 2^32, and a few rounds of batch-then-check at scale 14."""
import numpy as np
import pytest

from consumers_model import global_edges, last_slot_free, model_bfs, partition_states
from helpers import load_pkg
from paths_model import NO_PATH, assert_hard, global_edges_valued, hardness, model_components, model_sssp

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


def weigh(streams, ops, hi, seed):
    """the adds of `ops` with values in [1, hi] from the counter hash"""
    ops = ops.copy()
    w = (streams.uniform_ints(seed, len(ops), hi) + 1).astype(np.uint32)
    add = ops[:, 2] != 0
    ops[add, 2] = w[add]
    return ops


def check_model(pp, starts, label, hard_start=None):
    n = pp.get_n()
    states = partition_states(pp)
    src, dst, val = global_edges_valued(states)
    if hard_start is not None:
        lv, widest = model_bfs(src, dst, n, hard_start)
        h, ref = hardness(src, dst, val, n, hard_start, lv, widest)
        print(label, h)
        assert_hard(h, n, label)
        np.testing.assert_array_equal(pp.sssp(hard_start), ref, err_msg=f"{label}: sssp from {hard_start}")
    for s in starts:
        np.testing.assert_array_equal(pp.sssp(s), model_sssp(src, dst, val, n, s), err_msg=f"{label}: sssp from {s}")
    np.testing.assert_array_equal(pp.components(), model_components(src, dst, n), err_msg=f"{label}: components")
    after = partition_states(pp)  # nothing written
    for (_, i0, n0), (_, i1, n1) in zip(states, after):
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1), label


def busiest(pp):
    src, dst = global_edges(partition_states(pp))
    return int(np.bincount(src[dst < pp.get_n()]).argmax())


def test_paths_model_rmat18(pkg, streams):
    """P = 8: a 2 M-edge RMAT core with values in [1, 2^20] and a mixed stream, add_node, a repartition to balanced_starts;
    then a graph with a hub of 2^20 edges (wider than any wave walks on its own), bulk-built from a device tensor"""
    n, P = 1 << 18, 8
    s, d = streams.rmat_edges(18, 2_000_000, seed=31)
    core = weigh(streams, streams.adds(s, d), 1 << 20, seed=1)
    s2, d2 = streams.rmat_edges(18, 300_000, seed=32)
    mixed = weigh(streams, streams.mixed_existing_stream(core, streams.adds(s2, d2 + np.uint32(7)), seed=33), 1 << 20, seed=2)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    pp.apply(core)
    pp.apply(mixed)
    pp.add_node()
    pp.apply(np.array([[n, 1, 5], [2, n, 9]], np.uint32))
    pp.add_node()  # (isolated)
    main = busiest(pp)
    check_model(pp, [n // 2 + 5, n, n + 1], "rmat18", hard_start=main)
    pp.repartition(pp.balanced_starts())
    check_model(pp, [main, n - 1], "rmat18 repartitioned")
    pp.close()

    m, nh = 1 << 20, 1 << 21
    hub = 3 * nh // 8 + 11
    rng = np.random.default_rng(5)
    s3, d3 = streams.rmat_edges_folded(nh, 21, 2_000_000, seed=34)
    adds = np.concatenate([streams.adds(s3, d3), streams.adds(np.full(m, hub, np.uint32), rng.permutation(nh)[:m].astype(np.uint32))])
    adds = weigh(streams, adds, 1 << 20, seed=3)
    pp = pkg.PPPCSR(nh, numDomain=1, partitionsPerDomain=P)
    t = to_device(adds)
    pp.bulk_build_device(t.data_ptr(), len(adds))
    node = pp.getNode(hub)
    assert node[1] - node[0] > m
    check_model(pp, [hub, int(s3[0])], "hub")


def test_paths_match_one_engine_config2(pkg, streams):
    """config #2's graph (RMAT scale 20, 10 M core edges, bulk-built) and a 1 M mixed stream, on 8 partitions and on one
    PCSR: equal distances, equal labels"""
    n = 1 << 20
    s, d = streams.rmat_edges(20, 10_000_000, seed=1)
    core = weigh(streams, streams.adds(s, d), 1 << 20, seed=11)
    s2, d2 = streams.rmat_edges(20, 1_000_000, seed=2)
    mixed = weigh(streams, streams.mixed_existing_stream(core, streams.adds(s2, d2), seed=3), 1 << 20, seed=12)
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
    for start in (0, int(s[1]), n - 1):
        a, b = pp.sssp(start), one.sssp(start)
        np.testing.assert_array_equal(a, b)
    assert np.count_nonzero(pp.sssp(int(s[1])) != np.uint64(NO_PATH)) > n // 8  # (not a walk over a handful of vertices)
    la, lb = pp.components(), one.components()
    np.testing.assert_array_equal(la, lb)
    assert np.all(la <= np.arange(n, dtype=np.uint32)) and np.array_equal(la[la], la)


def test_sssp_values_near_2_32(pkg, streams):
    """values in [2^32 - 2^16, 2^32 - 2]: every path of two edges or more is longer than 2^32 (asserted from the model)"""
    n, P = 1 << 14, 4
    s, d = streams.rmat_edges(14, 120_000, seed=51)
    ops = streams.adds(s, d)
    ops[:, 2] = (np.uint64(0xFFFFFFFE) - streams.uniform_ints(5, len(ops), 1 << 16)).astype(np.uint32)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    pp.apply(ops)
    start = busiest(pp)
    src, dst, val = global_edges_valued(partition_states(pp))
    ref = model_sssp(src, dst, val, n, start)
    reached = ref != np.uint64(NO_PATH)
    assert int(ref[reached].max()) > 3 * 2 ** 32 and np.count_nonzero(ref[reached] > np.uint64(2 ** 32)) > n // 8
    np.testing.assert_array_equal(pp.sssp(start), ref)
    one = pkg.PCSR(n)
    one.apply(ops)
    np.testing.assert_array_equal(one.sssp(start), ref)


def test_paths_follow_batches(pkg, streams):
    """3 rounds of: apply a batch, then sssp and components against the model (scale 14)"""
    n, P = 1 << 14, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges(14, 60_000, seed=61)
    pp.apply(weigh(streams, streams.adds(s, d), 1000, seed=6))
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 20_000, seed=62 + r)
        batch = np.concatenate([weigh(streams, streams.adds(s2, d2), 1000, seed=70 + r),
                                streams.random_stream(n, 10_000, seed=80 + r, p_delete=0.5)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        check_model(pp, [busiest(pp), r * 1000 + 1], f"round {r}")
