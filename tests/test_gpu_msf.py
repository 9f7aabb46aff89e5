"""GPU: ppcsr_msf / pppcsr_msf on MI355X, all partitions on one device: the zoo of tests/msf_model.py and an RMAT scale-16
graph against the model (Kruskal on the distinct keys (w, lo, hi)) with the counters against the model's replica of the
schedule; closed forms on a ruler path, on an ascending-weight path of 2^18 vertices and on an array of 2^24 slots whose
streaming grids loop; and 8 partitions against one PCSR at config #2's size.  The schedule fixes passes = 2 * rounds - 1 and
host reads = rounds + pointer-jump launches + 1."""
import numpy as np
import pytest

from consumers_model import partition_states
from helpers import load_pkg
from msf_model import HARD, assert_hard, hardness, model_msf, ruler_path, zoo
from paths_model import global_edges_valued

pytestmark = pytest.mark.gpu

NO_EDGE = 0xFFFFFFFF
STREAM_GRID_SLOTS = 8192 * 4 * 256  # slots one step of the streaming grids covers once they stop growing: 8192 workgroups of 4 waves, 4 chunks of 64 slots each


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


def check_counters(c, hooks, n, count, label):
    """the counters of the last call against the model's rounds (hooks per hooking round; None: no model run)"""
    if hooks is not None:
        assert int(c[0]) == len(hooks) + 1 and int(c[4]) == (hooks[0] if hooks else 0) and sum(hooks) == count, (label, c, hooks)
        assert int(c[2]) >= len(hooks), (label, c)
    assert int(c[5]) == count and int(c[6]) == n - count, (label, c, count)
    assert int(c[0]) <= int(np.floor(np.log2(n))) + 1, (label, c)
    assert int(c[3]) <= int(np.ceil(np.log2(n))) + 1 and int(c[3]) <= int(c[2]), (label, c)
    assert int(c[1]) == 2 * int(c[0]) - 1, (label, c)  # the last round makes its first pass only
    assert int(c[7]) == int(c[0]) + int(c[2]) + 1 and c[7] >= c[0], (label, c)


def check_model(objs, label, **hard):
    """every object of objs (same edge set) against one model run: edges, weight, labels, components(), the counters, nothing written"""
    n = objs[0][1].get_n()
    src, dst, val = global_edges_valued(states_of(objs[0][1]))
    want_e, want_w, want_l = model_msf(src, dst, val, n)
    h = hardness(src, dst, val, n, want_e)
    print(label, h)
    assert_hard(h, label, **hard)
    for name, g in objs:
        before = states_of(g)
        s1, d1, v1 = global_edges_valued(before)
        assert np.array_equal(s1, src) and np.array_equal(d1, dst) and np.array_equal(v1, val), f"{label} {name}: another edge set"
        edges, weight, labels, ms = g.msf(with_ms=True)
        c = g.debug_msf_counters()
        print(f"{label} {name}: {ms:.2f} ms, counters {c.tolist()}")
        np.testing.assert_array_equal(edges.astype(np.int64), want_e, err_msg=f"{label} {name}: edges")
        assert weight == want_w, (label, name, weight, want_w)
        np.testing.assert_array_equal(labels, want_l, err_msg=f"{label} {name}: labels")
        np.testing.assert_array_equal(labels, g.components(), err_msg=f"{label} {name}: components")
        check_counters(c, h["hooks"], n, len(edges), f"{label} {name}")
        for (_, i0, n0), (_, i1, n1) in zip(before, states_of(g)):  # nothing written
            assert np.array_equal(i0, i1) and np.array_equal(n0, n1), (label, name)
    return want_e, want_w, want_l, h


def test_msf_zoo_and_batches(pkg, streams):
    """the zoo at n = 2^14 on 8 partitions and on one PCSR, then 3 rounds of batch-then-check"""
    n = 1 << 14
    ops = zoo(streams, n, 14, 60_000, seed=23)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    one = pkg.PCSR(n)
    for g in (pp, one):
        g.apply(ops)
    objs = [("P=8", pp), ("PCSR", one)]
    check_model(objs, "zoo", **HARD)
    for r in range(3):
        rng = np.random.default_rng(r)
        s2, d2 = streams.rmat_edges(14, 2_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 1_000, seed=80 + r, p_delete=0.5)])
        add = batch[:, 2] != 0
        batch[add, 2] = rng.integers(1, 5, int(add.sum()))
        batch = batch[rng.permutation(len(batch))]
        for g in (pp, one):
            g.apply(batch)
        check_model(objs, f"round {r}", ties=1, opposite=1, reverse_only=1, loops=1, beyond=1, isolated=1, rounds=3)
    pp.close()


def test_msf_model_rmat16(pkg, streams):
    """RMAT scale 16, 500 K edges with values in [1, 1000], on 8 partitions and on one PCSR: a mixed stream, add_node and edges
    to and from the new vertex, a repartition to balanced_starts"""
    n, P = 1 << 16, 8
    s, d = streams.rmat_edges(16, 500_000, seed=31)
    core = streams.adds(s, d)
    core[:, 2] = streams.uniform_ints(34, len(core), 1000) + 1
    s2, d2 = streams.rmat_edges(16, 80_000, seed=32)
    fresh = streams.adds(s2, d2 + np.uint32(7))
    fresh[:, 2] = streams.uniform_ints(35, len(fresh), 1000) + 1
    mixed = streams.mixed_existing_stream(core, fresh, seed=33)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    one = pkg.PCSR(n)
    for g in (pp, one):
        g.apply(core)
        g.apply(mixed)
        g.add_node()
        g.apply(np.array([[n, 1, 5], [2, n, 9]], np.uint32))
        g.add_node()  # (isolated)
    want_e, want_w, want_l, _ = check_model([("P=8", pp), ("PCSR", one)], "rmat16", **HARD)
    assert want_l[n + 1] == n + 1 and want_l[n] == want_l[1]
    pp.repartition(pp.balanced_starts())
    edges, weight, labels = pp.msf()
    np.testing.assert_array_equal(edges.astype(np.int64), want_e)
    assert weight == want_w
    np.testing.assert_array_equal(labels, want_l)
    pp.close()


@pytest.mark.parametrize("P", [1, 8])
def test_msf_ruler_path(pkg, P):
    """the ruler path on 2^16 permuted vertices, bulk-built: edge {i - 1, i} weighs 1 + ctz(i), so every round halves the
    components: exactly 16 hooking rounds and the empty one, hooks 2^15, ..., 2, 1; weight = 2^17 - 16 - 2"""
    k = 16
    n = 1 << k
    rng = np.random.default_rng(4)
    perm = rng.permutation(n).astype(np.int64)
    a, b, w = ruler_path(k)
    rows = np.stack([perm[a], perm[b], w], axis=1)
    flip = rng.integers(0, 2, len(rows)).astype(bool)  # stored in either direction
    rows[flip, :2] = rows[flip][:, [1, 0]]
    adds = rows.astype(np.uint32)[rng.permutation(len(rows))]
    g = pkg.PCSR(n) if P == 1 else pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    if P == 1:
        g.bulk_build(adds)
    else:
        t = to_device(adds)
        g.bulk_build_device(t.data_ptr(), len(adds))
        del t
    edges, weight, labels, ms = g.msf(with_ms=True)
    c = g.debug_msf_counters()
    print(f"ruler P={P}: {ms:.2f} ms, counters {c.tolist()}")
    want = np.stack([rows[:, :2].min(axis=1), rows[:, :2].max(axis=1), rows[:, 2]], axis=1)
    np.testing.assert_array_equal(edges.astype(np.int64), want[np.lexsort((want[:, 1], want[:, 0]))])
    assert weight == (1 << (k + 1)) - k - 2
    assert not labels.any()  # one tree, which holds vertex 0
    assert int(c[0]) == k + 1 and int(c[4]) == n // 2, c
    check_counters(c, [n >> (r + 1) for r in range(k)], n, n - 1, f"ruler P={P}")


def test_msf_ascending_path(pkg):
    """an ascending-weight path of L = 2^18 permuted vertices: every vertex but the light end's pair hooks towards the light end
    in ONE round, into one chain L - 1 deep, which pointer doubling flattens in at most ceil(log2 L) + 1 = 19 launches (a
    per-thread chase to the root would walk 2^18 links); weight = L (L - 1) / 2"""
    L = 1 << 18
    rng = np.random.default_rng(5)
    path = rng.permutation(L).astype(np.int64)
    rows = np.stack([path[:-1], path[1:], np.arange(1, L)], axis=1)
    g = pkg.PCSR(L)
    g.bulk_build(rows.astype(np.uint32)[rng.permutation(len(rows))])
    edges, weight, labels, ms = g.msf(with_ms=True)
    c = g.debug_msf_counters()
    print(f"ascending: {ms:.2f} ms, counters {c.tolist()}")
    assert weight == L * (L - 1) // 2 and len(edges) == L - 1 and not labels.any()
    want = np.stack([rows[:, :2].min(axis=1), rows[:, :2].max(axis=1), rows[:, 2]], axis=1)
    np.testing.assert_array_equal(edges.astype(np.int64), want[np.lexsort((want[:, 1], want[:, 0]))])
    assert int(c[0]) == 2 and int(c[4]) == L - 1 and int(c[3]) <= 19, c
    check_counters(c, [L - 1], L, L - 1, "ascending")


@pytest.mark.parametrize("P", [1, 8])
def test_msf_grid_stride_seam(pkg, P):
    """arrays of 2^24 slots in all, twice what one step of the streaming grids covers (they stop growing at 8192 workgroups),
    so every wave loops: n = 2^19, every block of 64 consecutive ids one path of weight 1 in a permuted order, 13 more pairs
    per vertex inside the block with weights in [2, 9] (a path pair wins where they coincide), one-way bridges of weight 5
    between some neighbouring blocks (block 4 i to 4 i + 1, block 4 i + 3 to 4 i + 2: no cycle).  Every pair beside the path
    closes a cycle of lighter path edges, so the forest is the paths and the bridges: weight = 63 n / 64 + 5 bridges, labels by
    block chain — without a model run.  On one PCSR a block's slots straddle slot 2^23, where the second step of the grids begins"""
    n, B = 1 << 19, 64
    rng = np.random.default_rng(9)
    order = rng.permuted(np.arange(n, dtype=np.int64).reshape(-1, B), axis=1)
    paths = np.stack([order[:, :-1].ravel(), order[:, 1:].ravel(), np.ones(n - n // B, np.int64)], axis=1)
    v = np.repeat(np.arange(n, dtype=np.int64), 13)
    more = np.stack([v, v - v % B + rng.integers(0, B, len(v)), rng.integers(2, 10, len(v))], axis=1)
    blocks = np.arange(0, n // B - 4, 4, dtype=np.int64)
    bridges = np.concatenate([np.stack([blocks * B + 5, (blocks + 1) * B + 9, np.full(len(blocks), 5)], axis=1),
                              np.stack([(blocks + 3) * B + 1, (blocks + 2) * B + 60, np.full(len(blocks), 5)], axis=1)])
    rows = np.concatenate([paths, bridges, more])  # (a bulk build takes distinct pairs: the first row of a pair is kept)
    _, first = np.unique(rows[:, 0] * n + rows[:, 1], return_index=True)
    adds = rows[np.sort(first)].astype(np.uint32)
    adds = adds[rng.permutation(len(adds))]
    forest = np.concatenate([paths, bridges])
    want = np.stack([forest[:, :2].min(axis=1), forest[:, :2].max(axis=1), forest[:, 2]], axis=1)
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    block = np.arange(n, dtype=np.int64) // B
    lead = np.where(block < n // B - 4, block - block % 2, block)  # blocks 4 i, 4 i + 1 are chained, and 4 i + 2, 4 i + 3; the last four stand alone
    want_l = (lead * B).astype(np.uint32)
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
        first_v = lo - lo % B
        assert g.getNode(first_v)[0] < STREAM_GRID_SLOTS < g.getNode(first_v + B - 1)[1], (lo, g.getNode(first_v), g.getNode(first_v + B - 1))
    else:
        g = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
        t = to_device(adds)
        g.bulk_build_device(t.data_ptr(), len(adds))
        del t
        slots = sum(g.partition(k).geometry()[0] for k in range(P))
    assert slots >= 2 * STREAM_GRID_SLOTS, slots
    edges, weight, labels, ms = g.msf(with_ms=True)
    c = g.debug_msf_counters()
    print(f"seam P={P}: {slots} slots, {ms:.2f} ms, counters {c.tolist()}")
    np.testing.assert_array_equal(edges.astype(np.int64), want)
    assert weight == 63 * n // 64 + 5 * len(bridges)
    np.testing.assert_array_equal(labels, want_l)
    check_counters(c, None, n, len(want), f"seam P={P}")


def test_msf_matches_one_engine_config2(pkg, streams):
    """config #2's size (RMAT scale 20, 10 M core edges bulk-built with values in [1, 2^20], then a 1 M mixed stream), on 8
    partitions and on one PCSR: equal outputs, and what can be checked without a Python model at this size.  A pair's value is
    a hash of the pair, so that the repeats of a pair in the core carry one value"""
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    n = 1 << 20

    def valued(s, d, salt):
        ops = streams.adds(s, d)
        ops[:, 2] = (streams.splitmix64(s.astype(np.uint64) * np.uint64(n) + d.astype(np.uint64) + np.uint64(salt)) % np.uint64(1 << 20)).astype(np.uint32) + 1
        return ops
    core = valued(*streams.rmat_edges(20, 10_000_000, seed=1), salt=0)
    mixed = streams.mixed_existing_stream(core, valued(*streams.rmat_edges(20, 1_000_000, seed=2), salt=1 << 50), seed=3)
    one = pkg.PCSR(n)
    one.bulk_build(core)
    one.apply(mixed)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    t = to_device(core)
    pp.bulk_build_device(t.data_ptr(), len(core))
    del t
    pp.apply(mixed)
    (ea, wa, la, ma), (eb, wb, lb, mb) = pp.msf(with_ms=True), one.msf(with_ms=True)
    ca, cb = pp.debug_msf_counters(), one.debug_msf_counters()
    print(f"config2: P=8 {ma:.2f} ms {ca.tolist()}, PCSR {mb:.2f} ms {cb.tolist()}")
    np.testing.assert_array_equal(ea, eb)
    assert wa == wb == sum(int(x) for x in ea[:, 2].astype(np.int64).tolist())
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ca[:2], cb[:2])
    np.testing.assert_array_equal(ca[4:7], cb[4:7])
    ids = np.arange(n, dtype=np.uint32)
    np.testing.assert_array_equal(la, one.components())
    assert len(ea) == n - int((la == ids).sum())
    check_counters(ca, None, n, len(ea), "config2 P=8")
    check_counters(cb, None, n, len(eb), "config2 PCSR")
    # ascending by (lo, hi), lo < hi; every edge is stored with its value in at least one direction, with no smaller value in the other
    key = ea[:, 0].astype(np.int64) * n + ea[:, 1]
    assert np.all(ea[:, 0] < ea[:, 1]) and np.all(key[1:] > key[:-1])
    f, r = one.lookup_edges(ea[:, 0], ea[:, 1]), one.lookup_edges(ea[:, 1], ea[:, 0])
    assert np.all((f == ea[:, 2]) | (r == ea[:, 2]))
    assert np.all((f == NO_EDGE) | (f >= ea[:, 2])) and np.all((r == NO_EDGE) | (r >= ea[:, 2]))
    # the returned edges alone connect exactly what the labels say
    m = sp.coo_matrix((np.ones(len(ea)), (ea[:, 0], ea[:, 1])), shape=(n, n)).tocsr()
    ncomp, lab = csgraph.connected_components(m, directed=False)
    assert ncomp == n - len(ea)  # (a forest: every edge joins two trees)
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    np.testing.assert_array_equal(smallest[lab], la)
    pp.close()
