"""GPU: ppcsr_scc / pppcsr_scc on MI355X, all partitions on one device: the zoo of tests/scc_model.py and an RMAT scale-16
graph against the model (an iterative Tarjan on Python integers) with the counters of every phase, a closed form on an array
of 2^24 slots whose streaming grids loop, and 8 partitions against one PCSR at config #2's size."""
import numpy as np
import pytest

from consumers_model import global_edges, partition_states
from helpers import load_pkg
from scc_model import assert_hard, hardness, model_scc, trim_closure, zoo

pytestmark = pytest.mark.gpu

NO_PIVOT = 0xFFFFFFFFFFFFFFFF
STREAM_GRID_SLOTS = 8192 * 4 * 256  # slots one step of the streaming grids covers once they stop growing: 8192 workgroups of 4 waves, 4 chunks of 64 slots each
ZOO = dict(n=1 << 14, scale=14, core_edges=60_000, cycles=24, longest=700, k=40, L=1500)
ZOO_HARD = dict(nontrivial=60, distinct=10, largest=2000, trim_sweeps=500, below=1, above=1, loops=4, beyond=1)


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


def states_of(g):
    if hasattr(g, "num_partitions"):
        return partition_states(g)
    items, nodes = g.state()
    return [(0, items, nodes)]


def counters_of(g):
    return g.debug_scc_counters()


def check_model(objs, label, colouring=None, **hard):
    """every object of objs (same edge set) against one model run: labels, count, the counter conditions, nothing written"""
    n = objs[0][1].get_n()
    states = states_of(objs[0][1])
    src, dst = global_edges(states)
    want = model_scc(src, dst, n)
    h = hardness(src, dst, n, want)
    print(label, h)
    assert_hard(h, label, **hard)
    closure = int(trim_closure(src, dst, n)[0].sum())
    for name, g in objs:
        before = states_of(g)
        s1, d1 = global_edges(before)
        assert np.array_equal(s1, src) and np.array_equal(d1, dst), f"{label} {name}: another edge set"
        labels, count, ms = g.scc(with_ms=True)
        np.testing.assert_array_equal(labels, want, err_msg=f"{label} {name}: labels")
        assert count == int((want == np.arange(n)).sum()), (label, name, count)
        c = counters_of(g)
        print(f"{label} {name}: {ms:.2f} ms, counters {c.tolist()}")
        assert int(c[0] + c[3] + c[5]) == n, (label, name, c)
        assert c[2] != NO_PIVOT and int(c[3]) == int((want == want[int(c[2])]).sum()), (label, name, c)
        assert int(c[0]) >= closure and c[1] >= 1, (label, name, c, closure)
        if colouring is True:
            assert c[4] >= 1 and c[5] >= 1, (label, name, c)
        if colouring is False:
            assert h["nontrivial"] == 1 and c[4] == 0 and c[5] == 0 and int(c[3]) == h["largest"], (label, name, c, h)
        for (_, i0, n0), (_, i1, n1) in zip(before, states_of(g)):  # nothing written
            assert np.array_equal(i0, i1) and np.array_equal(n0, n1), (label, name)
    return want, h


def test_scc_zoo_and_batches(pkg, streams):
    """the zoo at n = 2^14 on 8 partitions and on one PCSR, then 3 rounds of batch-then-check.  The first call makes 5436
    passes over small arrays, each with its host read (791 trim sweeps, 40 colouring rounds, 5479 reads).  Observed on one
    MI355X: 153 ms of device time for that call on one PCSR and 169 ms on 8 partitions, about 30 us per pass with its read;
    4 to 12 ms for the calls after the batches (129 to 363 passes); the whole test 1.1 s"""
    n = ZOO["n"]
    ops = zoo(streams, seed=23, **ZOO)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    one = pkg.PCSR(n)
    for g in (pp, one):
        g.apply(ops)
    objs = [("P=8", pp), ("PCSR", one)]
    check_model(objs, "zoo", colouring=True, **ZOO_HARD)
    assert counters_of(pp)[4] >= ZOO["k"]  # the ascending chain of two-cycles: one round each
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 2_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 1_000, seed=80 + r, p_delete=0.5)])
        batch = batch[np.random.default_rng(r).permutation(len(batch))]
        for g in (pp, one):
            g.apply(batch)
        check_model(objs, f"round {r}", nontrivial=2)
    pp.close()


def test_scc_model_rmat16(pkg, streams):
    """RMAT scale 16, 500 K edges, on 8 partitions and on one PCSR: a mixed stream, add_node and edges to and from the new
    vertex, a repartition to balanced_starts.  One giant SCC and single vertices: trimming and one pivot label everything"""
    n, P = 1 << 16, 8
    s, d = streams.rmat_edges(16, 500_000, seed=31)
    core = streams.adds(s, d)
    s2, d2 = streams.rmat_edges(16, 80_000, seed=32)
    mixed = streams.mixed_existing_stream(core, streams.adds(s2, d2 + np.uint32(7)), seed=33)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    one = pkg.PCSR(n)
    for g in (pp, one):
        g.apply(core)
        g.apply(mixed)
        g.add_node()
        g.apply(np.array([[n, 1, 5], [2, n, 9]], np.uint32))
        g.add_node()  # (isolated)
    objs = [("P=8", pp), ("PCSR", one)]
    want, _ = check_model(objs, "rmat16", colouring=False, largest=n // 8, beyond=1)
    assert want[n + 1] == n + 1
    pp.repartition(pp.balanced_starts())
    check_model([("P=8 repartitioned", pp)], "rmat16", colouring=False, largest=n // 8)
    pp.close()


@pytest.mark.parametrize("P", [1, 8])
def test_scc_grid_stride_seam(pkg, P):
    """arrays of 2^24 slots in all, twice what one step of the streaming grids covers (they stop growing at 8192 workgroups),
    so every wave loops: n = 2^19, every block of 64 consecutive ids one directed cycle in a permuted order plus 13 more edges
    per vertex inside the block, one-way bridges between some neighbouring blocks (up from every block 4 i, down into every
    block 4 i + 2).  labels[v] = v - v % 64, without a model run.  No vertex can be trimmed, one block goes to the pivot, the
    rest to colouring.  On one PCSR a block's slots straddle slot 2^23, where the second step of the grids begins"""
    n, B = 1 << 19, 64
    rng = np.random.default_rng(9)
    order = rng.permuted(np.arange(n, dtype=np.int64).reshape(-1, B), axis=1)
    rows = [np.stack([order.ravel(), np.roll(order, -1, axis=1).ravel()], axis=1)]
    v = np.repeat(np.arange(n, dtype=np.int64), 13)
    rows.append(np.stack([v, v - v % B + rng.integers(0, B, len(v))], axis=1))
    blocks = np.arange(0, n // B - 4, 4, dtype=np.int64)
    rows.append(np.stack([blocks * B + 5, (blocks + 1) * B + 9], axis=1))
    rows.append(np.stack([(blocks + 3) * B + 1, (blocks + 2) * B + 60], axis=1))
    rows = np.concatenate(rows)
    key = np.unique(rows[:, 0] * n + rows[:, 1])  # (a bulk build takes distinct pairs)
    adds = np.stack([key // n, key % n, np.ones(len(key), np.int64)], axis=1).astype(np.uint32)
    adds = adds[rng.permutation(len(adds))]
    want = (np.arange(n) - np.arange(n) % B).astype(np.uint32)
    if P == 1:
        g = pkg.PCSR(n)
        g.bulk_build(adds)
        slots = g.geometry()[0]
        lo, hi = 0, n - 1  # the first vertex whose range ends beyond the seam
        while lo < hi:
            mid = (lo + hi) // 2
            if g.getNode(mid)[1] > STREAM_GRID_SLOTS:
                hi = mid
            else:
                lo = mid + 1
        first = lo - lo % B
        assert g.getNode(first)[0] < STREAM_GRID_SLOTS < g.getNode(first + B - 1)[1], (lo, g.getNode(first), g.getNode(first + B - 1))
    else:
        g = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
        t = to_device(adds)
        g.bulk_build_device(t.data_ptr(), len(adds))
        del t
        slots = sum(g.partition(k).geometry()[0] for k in range(P))
    assert slots >= 2 * STREAM_GRID_SLOTS, slots
    labels, count, ms = g.scc(with_ms=True)
    c = counters_of(g)
    print(f"seam P={P}: {slots} slots, {ms:.2f} ms, counters {c.tolist()}")
    np.testing.assert_array_equal(labels, want)
    assert count == n // B
    assert c[0] == 0 and c[3] == B and c[4] >= 1 and int(c[5]) == n - B, c


def test_scc_matches_one_engine_config2(pkg, streams):
    """config #2's graph (RMAT scale 20, 10 M core edges, bulk-built) and a 1 M mixed stream, on 8 partitions and on one
    PCSR: equal labels and counts, and the invariants of the label convention (no Python model at this size)"""
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
    (la, ca, ma), (lb, cb, mb) = pp.scc(with_ms=True), one.scc(with_ms=True)
    print(f"config2: P=8 {ma:.2f} ms {counters_of(pp).tolist()}, PCSR {mb:.2f} ms {counters_of(one).tolist()}")
    np.testing.assert_array_equal(la, lb)
    ids = np.arange(n, dtype=np.uint32)
    assert ca == cb == int((la == ids).sum())
    assert np.all(la <= ids) and np.array_equal(la[la], la)
    assert int(np.bincount(la).max()) > n // 8  # the largest SCC
    comp = one.components()
    assert np.array_equal(comp[la], comp)  # SCC labels refine WCC labels
    pp.close()
