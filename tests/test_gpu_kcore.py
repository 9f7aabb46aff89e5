"""GPU: ppcsr_kcore / pppcsr_kcore on MI355X, all partitions on one device: against the model of tests/kcore_model.py
(Batagelj-Zaversnik bucket peeling, computed on the host) at RMAT scale 14 under streams and a repartition, once at scale 18
on 8 partitions and on one PCSR, and a few rounds of batch-then-check."""
import ctypes

import numpy as np
import pytest

from consumers_model import global_edges, partition_states
from helpers import load_pkg
from kcore_model import assert_hard, hardness, model_kcore

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


def check_model(pp, label, **hard):
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    want = model_kcore(src, dst, n)
    h = hardness(src, dst, n, want)
    assert_hard(h, label, **hard)
    core, kmax, ms = pp.kcore(with_ms=True)
    np.testing.assert_array_equal(core, want, err_msg=f"{label}: core")
    assert kmax == h["kmax"] and ms >= 0.0, (label, kmax, h)
    for (_, i0, n0), (_, i1, n1) in zip(states, partition_states(pp)):  # nothing written
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1), label
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return want, h


def test_kcore_model_rmat14(pkg, streams):
    """P = 8: an RMAT core, a mixed stream over stored and fresh pairs with destinations >= n, add_node and edges to and from
    the new vertex, a repartition to balanced_starts"""
    n, P = 1 << 14, 8
    hard = dict(kmax=24, distinct=24, gaps=1, max_subrounds=4, below_degree=n // 16, backward=1, loops=1, beyond=1)
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
    want, _ = check_model(pp, "rmat14 add_node", **hard)
    assert want[n] >= 2
    pp.repartition(pp.balanced_starts())
    check_model(pp, "rmat14 repartitioned", **hard)
    pp.close()


def test_kcore_model_rmat18(pkg, streams):
    """once at scale 18, bulk-built from a device tensor on 8 partitions and on one PCSR: a first frontier beyond the grid's
    waves, lists beyond one wave's reach, more than a hundred levels with gaps between them"""
    n = 1 << 18
    s, d = streams.rmat_edges(18, 2_000_000, seed=31)
    adds = streams.adds(s, d)
    t = to_device(adds)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    pp.bulk_build_device(t.data_ptr(), len(adds))
    one = pkg.PCSR(n)
    one.bulk_build(adds)
    del t
    want, h = check_model(pp, "rmat18", widest=1 << 16, maxdeg=4097, kmax=64, gaps=1, max_subrounds=8)
    core, kmax = one.kcore()
    np.testing.assert_array_equal(core, want)
    assert kmax == h["kmax"]
    pp.close()


def test_kcore_follow_batches(pkg, streams):
    """3 rounds of: apply a batch of adds, deletes, a self-loop and a destination >= n, then kcore against the model"""
    n, P = 1 << 14, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges(14, 60_000, seed=61)
    pp.apply(streams.adds(s, d))
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 20_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 10_000, seed=80 + r, p_delete=0.5),
                                np.array([[r, r, 1], [r, n + r, 1]], np.uint32)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        check_model(pp, f"round {r}", kmax=16, distinct=16, backward=1, loops=1, beyond=1)
    pp.close()


def test_kcore_status_codes(pkg, streams):
    """argument errors with EINVAL; partitions on two devices refused with EUNSUPPORTED; the sequential regime answered"""
    n = 1 << 12
    s, d = streams.rmat_edges(12, 60_000, seed=41)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4)
    pp.apply(streams.adds(s, d))
    L = pp.L
    core = np.empty(n, np.uint32)
    kmax = ctypes.c_uint32(77)
    e = pp.partition(2)
    assert L.pppcsr_kcore(pp.h, None, None, None) == 1
    assert L.pppcsr_kcore(None, core.ctypes.data, ctypes.byref(kmax), None) == 1
    assert L.ppcsr_kcore(e.h, None, None, None) == 1
    assert L.ppcsr_kcore(None, core.ctypes.data, None, None) == 1
    src, dst = global_edges(partition_states(pp))
    want = model_kcore(src, dst, n)
    assert L.pppcsr_kcore(pp.h, None, ctypes.byref(kmax), None) == 0 and kmax.value == want.max() >= 16
    assert L.pppcsr_kcore(pp.h, core.ctypes.data, None, None) == 0
    np.testing.assert_array_equal(core, want)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    tri = np.empty(n, np.uint64)
    assert L.pppcsr_triangles(pp.h, tri.ctypes.data, None, None) == 4  # (the regime triangles refuses)
    got, top = pp.kcore()
    np.testing.assert_array_equal(got, want)
    assert top == want.max()
    part, _ = e.kcore()
    assert len(part) == e.get_n()
    e.set_option("search_narrow", 1)
    if L.ppcsr_device_count() >= 2:
        two = pkg.PPPCSR(n, numDomain=2, partitionsPerDomain=1, devices=[0, 1])
        assert L.pppcsr_kcore(two.h, core.ctypes.data, ctypes.byref(kmax), None) == 4
        assert "more than one device" in L.ppcsr_last_error().decode()
