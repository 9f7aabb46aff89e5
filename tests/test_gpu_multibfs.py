"""GPU: ppcsr_multi_bfs / pppcsr_multi_bfs on one PCSR and on 8 partitions with the same edges.  Every output is compared
exactly — harmonic bit for bit — with tests/multibfs_model.py and every levels row with the device's own bfs; the counters of
ppcsr_debug_multi_bfs_counters and the model's histograms show that the listed edge step, the streaming pass and the pass that
finishes a hub all ran, so that nothing passes for want of work."""
import numpy as np
import pytest

from consumers_model import NO_LEVEL, global_edges
from helpers import load_pkg
from multibfs_checks import One, assert_equals_model, check
from multibfs_model import aggregates, hist_of, model_multi_bfs
from test_gpu_scc import STREAM_GRID_SLOTS, states_of, to_device

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 4
N = 1 << 14
PATH0, PATH_LEN, HUB, STAR, LOOP, BEYOND = 1000, 700, 5, 7, 30, 31
LONE = (20, 21, 22, 23)


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()
    return p


def zoo(streams, seed=3):
    """n = 2^14: a directed path of 700 vertices that nothing else enters (deep levels, the listed step), a hub with 6000 distinct
    out-neighbours (a slot range beyond what one wave walks), a star of 200, four isolated vertices, a vertex whose only edge is a
    self-loop, a vertex whose edges all leave the graph, and 60 K RMAT edges around them"""
    rng = np.random.default_rng(seed)
    inner = np.arange(PATH0 + 1, PATH0 + PATH_LEN)
    special = np.concatenate([inner, LONE, [LOOP, BEYOND]])
    free = np.setdiff1d(np.arange(N), special)
    s, d = streams.rmat_edges(14, 60_000, seed=seed)
    keep = ~np.isin(d, special) & ~np.isin(s, np.concatenate([LONE, [LOOP, BEYOND]]))
    rows = [np.stack([s[keep], d[keep]], 1).astype(np.int64),
            np.stack([np.arange(PATH0, PATH0 + PATH_LEN - 1), np.arange(PATH0 + 1, PATH0 + PATH_LEN)], 1),
            np.stack([np.full(6000, HUB), rng.permutation(free)[:6000]], 1),
            np.stack([np.full(200, STAR), rng.permutation(free)[:200]], 1),
            np.array([[LOOP, LOOP], [BEYOND, N + 1], [BEYOND, N + 5]])]
    rows = np.concatenate(rows)
    ops = np.concatenate([rows, np.ones((len(rows), 1), np.int64)], 1).astype(np.uint32)
    return ops[rng.permutation(len(ops))]


def zoo_sources(seed=4):
    """k = 130: two groups of 64 distinct vertices from all over the id range (a pass at level 0) that hold the star's centre, the
    degenerate vertices and the path's head, one of them twice; the last group is the hub and the path's head alone (listed
    steps, the hub left to a pass)"""
    rng = np.random.default_rng(seed)
    s = rng.permutation(N)[:128].astype(np.uint32)
    s[[0, 1, 2, 3, 4, 5, 70, 127]] = [STAR, LONE[0], LOOP, BEYOND, PATH0, PATH0 + PATH_LEN - 1, LONE[1], N - 1]
    s = np.concatenate([s, [HUB, PATH0]]).astype(np.uint32)
    s[100] = s[64]  # a repeated source inside one group
    return s


def check_all(objs, sources, label, bfs_rows=None):
    """every object of objs (same edge set) against ONE model run: all outputs, rows against bfs, nothing written, and the
    objects word for word alike; returns (model, counters per object)"""
    n = objs[0][1].get_n()
    src, dst = global_edges(states_of(objs[0][1]))
    m = model_multi_bfs(src, dst, n, sources)
    ctrs, gots = [], []
    for name, g in objs:
        before = states_of(g)
        s1, d1 = global_edges(before)
        assert np.array_equal(s1, src) and np.array_equal(d1, dst), f"{label} {name}: another edge set"
        assert_equals_model(g.multi_bfs(sources), m, f"{label} {name} (aggregates only)")
        got = g.multi_bfs(sources, levels=True, with_ms=True)
        c = g.debug_multi_bfs_counters()
        print(f"{label} {name}: {got[5]:.2f} ms, counters {c.tolist()}")
        assert_equals_model(got[:5], m, f"{label} {name}")
        rows = range(len(sources)) if bfs_rows is None else bfs_rows
        for i in rows:
            np.testing.assert_array_equal(got[4][i], g.bfs(int(sources[i])), err_msg=f"{label} {name}: row {i} against bfs")
        for (_, i0, n0), (_, i1, n1) in zip(before, states_of(g)):  # nothing written
            assert np.array_equal(i0, i1) and np.array_equal(n0, n1), (label, name)
        ctrs.append(c)
        gots.append(got)
    for a, b in zip(gots[0][:5], gots[-1][:5]):
        np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
    return m, ctrs


def test_multibfs_zoo_and_batches(pkg, streams):
    """the zoo on 8 partitions and on one PCSR, k = 130, then 3 rounds of batch-then-check"""
    ops = zoo(streams)
    sources = zoo_sources()
    pp = pkg.PPPCSR(N, numDomain=1, partitionsPerDomain=8)
    one = pkg.PCSR(N)
    for g in (pp, one):
        g.apply(ops)
    node = one.getNode(HUB)
    assert node[1] - node[0] - 1 > 4096, node
    owners = {int(np.searchsorted([pp.partition_start(k) for k in range(8)], int(s), side="right")) for s in sources}
    assert len(owners) == 8  # sources in every partition
    objs = [("P=8", pp), ("PCSR", one)]
    m, ctrs = check_all(objs, sources, "zoo")
    for c in ctrs:  # the conditions that keep the test from passing for want of work
        assert c[0] == 3 and c[3] >= 1 and c[2] >= 1 and c[4] >= 1, c
        assert c[3] >= PATH_LEN - 1 and c[5] >= 64 and c[6] == c[2] + c[3], c
    assert max(m["ecc"]) >= PATH_LEN - 1 and min(m["reached"]) == 1
    assert m["reached"][1] == 1 and m["reached"][2] == 1 and m["reached"][3] == 1  # isolated, self-loop only, edges that leave
    assert m["ecc"][129] >= PATH_LEN - 1 and m["reached"][128] >= 6001 and m["hists"][0][1] >= 200
    assert m["hists"][100] == m["hists"][64]  # the repeated source
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 2_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(N, 1_000, seed=80 + r, p_delete=0.5)])
        batch = batch[np.random.default_rng(r).permutation(len(batch))]
        for g in (pp, one):
            g.apply(batch)
        check_all(objs, sources, f"round {r}", bfs_rows=range(0, 130, 9))
    pp.close()


def test_multibfs_regimes_and_refusals(pkg, streams):
    """the sequential regime (narrow == 0 on one partition) answers from streaming passes alone; after a batch has ended it the
    rows equal bfs again; every refusal comes back with the output buffers untouched"""
    n, P, k = 3000, 4, 70
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges_folded(n, 12, 20_000, seed=50)
    pp.apply(streams.adds(s, d))
    L, e = pp.L, pp.partition(2)
    rng = np.random.default_rng(5)
    q = rng.integers(0, n, k).astype(np.uint32)
    Q = q.ctypes.data
    lv = np.full((k, n), 77, np.uint32)
    reached, far = np.full(k, 77, np.uint64), np.full(k, 77, np.uint64)
    ecc, harm = np.full(k, 77, np.uint32), np.full(k, 77.0, np.float64)
    outs = [b.ctypes.data for b in (lv, reached, far, ecc, harm)]
    for fn, h, m_n in ((L.pppcsr_multi_bfs, pp.h, n), (L.ppcsr_multi_bfs, e.h, e.get_n())):
        qq = (q % m_n).astype(np.uint32)
        assert fn(None, qq.ctypes.data, k, *outs, None) == EINVAL
        assert fn(h, None, k, *outs, None) == EINVAL
        assert fn(h, qq.ctypes.data, k, None, None, None, None, None, None) == EINVAL
        bad = qq.copy()
        bad[k - 1] = m_n
        assert fn(h, bad.ctypes.data, k, *outs, None) == EINVAL and "out of range" in L.ppcsr_last_error().decode()
        assert fn(h, None, 0, None, None, None, None, None, None) == 0  # k == 0: nothing to read or write
        assert fn(h, qq.ctypes.data, 0, *outs, None) == 0
    assert np.all(lv == 77) and np.all(reached == 77) and np.all(far == 77) and np.all(ecc == 77) and np.all(harm == 77.0)
    e.set_option("search_narrow", 0)  # the sequential regime, as the sampling tests reach it
    assert e.stats()["narrow"] == 0
    _, _, c = check(pp, q, "sequential", bfs_rows=0)
    print("sequential:", c.tolist())
    assert c[3] == 0 and c[4] == 0 and c[2] == c[1] and c[2] >= 2, c
    _, _, c = check(One(e), (q % e.get_n()).astype(np.uint32), "sequential, one engine", bfs_rows=0)
    assert c[3] == 0 and c[4] == 0, c
    assert e.stats()["narrow"] == 0
    pp.apply(streams.random_stream(n, 2000, seed=52, p_delete=0.3))  # (the range check runs: the regime ends)
    assert e.stats()["narrow"] == 1
    _, _, c = check(pp, q, "after the regime", bfs_rows=None)
    assert c[3] >= 1, c
    if L.ppcsr_device_count() >= 2:
        two = pkg.PPPCSR(n, numDomain=2, partitionsPerDomain=1, devices=[0, 1])
        reached[:] = 77
        assert L.pppcsr_multi_bfs(two.h, Q, k, None, outs[1], None, None, None, None) == EUNSUPPORTED
        assert "more than one device" in L.ppcsr_last_error().decode() and np.all(reached == 77)
        two.close()
    pp.close()


@pytest.mark.parametrize("P", [1, 8])
def test_multibfs_vertex_grid_seam(pkg, P):
    """n = 2^20 + 4133: the per-vertex grids stop growing at 4096 workgroups of 256 threads = 2^20, so the vertex step and the
    bitmap sweep loop for the last 4133 vertices.  Edges v -> v + 2^20 for v < 4133 and 0 -> v for v in [1, 4133), bulk-built:
    from 0, level 1 is [1, 4133) and 2^20, level 2 is 2^20 + [1, 4133); from 5 only 2^20 + 5; from 2^20 + 7 nothing"""
    M, T = 1 << 20, 4133
    n = M + T
    v = np.arange(T, dtype=np.int64)
    rows = np.concatenate([np.stack([v, v + M], 1), np.stack([np.zeros(T - 1, np.int64), v[1:]], 1)])
    adds = np.concatenate([rows, np.ones((len(rows), 1), np.int64)], 1).astype(np.uint32)
    adds = adds[np.random.default_rng(2).permutation(len(adds))]
    if P == 1:
        g = pkg.PCSR(n)
        g.bulk_build(adds)
    else:
        g = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
        t = to_device(adds)
        g.bulk_build_device(t.data_ptr(), len(adds))
        del t
    sources = np.array([0, 5, M + 7], np.uint32)
    reached, far, ecc, harm, lv, ms = g.multi_bfs(sources, levels=True, with_ms=True)
    print(f"vertex seam P={P}: {ms:.2f} ms, counters {g.debug_multi_bfs_counters().tolist()}")
    want = np.full((3, n), NO_LEVEL, np.uint32)
    want[0, 0], want[0, 1:T], want[0, M], want[0, M + 1:M + T] = 0, 1, 1, 2
    want[1, 5], want[1, M + 5] = 0, 1
    want[2, M + 7] = 0
    np.testing.assert_array_equal(lv, want)
    assert reached.tolist() == [2 * T, 2, 1] and far.tolist() == [T + 2 * (T - 1), 1, 0] and ecc.tolist() == [2, 1, 0]
    assert harm.tolist() == [float(T) + float(T - 1) / 2.0, 1.0, 0.0]
    got = g.multi_bfs(sources)
    for a, b in zip(got, (reached, far, ecc, harm)):
        np.testing.assert_array_equal(a, b)
    if P != 1:
        g.close()


@pytest.fixture(scope="module")
def rmat19(streams):
    """RMAT scale 19, 8 M adds: 7 611 111 distinct pairs (generated once for both forms)"""
    n = 1 << 19
    s, d = streams.rmat_edges(19, 8_000_000, seed=77)
    key = np.unique(s.astype(np.int64) * n + d.astype(np.int64))  # (a bulk build takes distinct pairs)
    src, dst = key // n, key % n
    return n, src, dst, np.stack([src, dst, np.ones(len(key), np.int64)], axis=1).astype(np.uint32)


@pytest.mark.parametrize("P", [1, 8])
def test_multibfs_stream_grid_seam(pkg, rmat19, P):
    """arrays of at least 2^24 slots in all, twice what one step of the streaming grid covers, so every wave of the pass loops:
    RMAT scale 19, about 7.6 M distinct edges, bulk-built; 64 sources with an out-edge.  Every row against the device's bfs, the
    aggregates recomputed from those rows, two sources against the model over the edge list"""
    n, src, dst, adds = rmat19
    if P == 1:
        g = pkg.PCSR(n)
        g.bulk_build(adds)
        slots = g.geometry()[0]
    else:
        g = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
        t = to_device(adds)
        g.bulk_build_device(t.data_ptr(), len(adds))
        del t
        slots = sum(g.partition(k).geometry()[0] for k in range(P))
    assert slots >= 2 * STREAM_GRID_SLOTS, (slots, len(adds))
    rng = np.random.default_rng(11)
    sources = rng.choice(np.unique(src), 64, replace=False).astype(np.uint32)
    reached, far, ecc, harm, lv, ms = g.multi_bfs(sources, levels=True, with_ms=True)
    c = g.debug_multi_bfs_counters()
    print(f"stream seam P={P}: {len(adds)} edges, {slots} slots, {ms:.2f} ms, counters {c.tolist()}")
    assert c[0] == 1 and c[2] >= 1, c
    for i, v in enumerate(sources):
        row = g.bfs(int(v))
        np.testing.assert_array_equal(lv[i], row, err_msg=f"row {i} against bfs({v})")
        r, f, e, h = aggregates(hist_of(row))
        assert (int(reached[i]), int(far[i]), int(ecc[i])) == (r, f, e), i
        assert harm[i:i + 1].view(np.uint64)[0] == np.array([h]).view(np.uint64)[0], i
    m = model_multi_bfs(src, dst, n, sources[[0, 63]])
    assert_equals_model((reached[[0, 63]], far[[0, 63]], ecc[[0, 63]], harm[[0, 63]], lv[[0, 63]]), m, "against the model")
    assert max(m["reached"]) > n // 4
    if P != 1:
        g.close()
