"""GPU (MI355X): the batched reads on real states — config #2's graph (RMAT scale 20, 10 M-edge core) plus 1 M mixed
updates checked against the oracle, a bulk-built hub of 2^22 edges, PPPCSR with 8 partitions on one GPU, the device forms
through torch tensors, and lookups interleaved with batches.  Answers are compared with a numpy model of the exported state
(sorted src << 32 | dst keys + np.searchsorted for lookups, the live slots of each vertex's range for gathers)."""
import numpy as np
import pytest

from helpers import _live, load_pkg, model_gather, model_lookup
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

NO_EDGE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()
    return p


def check_queries(e, rng, n_lookup, n_gather, label):
    items, nodes = e.state()
    n = len(nodes)
    live = np.nonzero(_live(items))[0]
    half = n_lookup // 2
    pick = items[live[rng.integers(0, len(live), half)]]
    rs = np.concatenate([pick[:, 0], rng.integers(0, n + n // 16, n_lookup - half).astype(np.uint32)])
    rd = np.concatenate([pick[:, 1], rng.integers(0, n, n_lookup - half).astype(np.uint32)])
    perm = rng.permutation(n_lookup)
    qs, qd = rs[perm].astype(np.uint32), rd[perm].astype(np.uint32)
    got = e.lookup_edges(qs, qd)
    want = model_lookup(items, n, qs, qd)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{label}: {len(bad)} lookups differ, first {[(int(qs[j]), int(qd[j]), int(got[j]), int(want[j])) for j in bad[:5]]}"
    assert np.mean(got != NO_EDGE) > 0.45
    for j in rng.choice(n_lookup, 64, replace=False):  # the single call on a sample
        if qs[j] < n:
            assert e.edge_exists(int(qs[j]), int(qd[j])) == (got[j] != NO_EDGE)
    verts = rng.integers(0, n + 64, n_gather).astype(np.uint32)
    rows, dests, vals = e.gather_neighbourhoods(verts)
    wr, wd, wv = model_gather(items, nodes, verts)
    np.testing.assert_array_equal(rows, wr, err_msg=label)
    np.testing.assert_array_equal(dests, wd, err_msg=label)
    np.testing.assert_array_equal(vals, wv, err_msg=label)
    for v in rng.choice(verts[verts < n], 16):
        i = int(np.nonzero(verts == v)[0][0])
        np.testing.assert_array_equal(dests[int(rows[i]):int(rows[i + 1])], e.get_neighbourhood(int(v)))
    return items, nodes


def test_config2_graph_lookups_and_gathers(pkg, streams):
    n = 1 << 20
    s, d = streams.rmat_edges(20, 10_000_000, seed=1)
    core = streams.adds(s, d)
    e, o = pkg.PCSR(n), Oracle(n)
    e.apply(core)
    s2, d2 = streams.rmat_edges(20, 1_000_000, seed=2)
    upd = streams.mixed_existing_stream(core, streams.adds(s2, d2)[:500_000], seed=3)
    e.apply(upd)
    o.apply(core)
    o.apply(upd)
    ei, en = e.state()
    oi, on = o.state()
    assert e.geometry() == o.geometry()
    np.testing.assert_array_equal(en, on)
    np.testing.assert_array_equal(ei, oi)
    st = e.stats()
    items, nodes = check_queries(e, np.random.default_rng(1), 1 << 22, 1 << 20, "config #2 + 1 M mixed")
    assert e.stats() == st
    i2, n2 = e.state()
    assert np.array_equal(i2, items) and np.array_equal(n2, nodes)
    # the device forms through torch tensors
    import torch
    rng = np.random.default_rng(2)
    qs = rng.integers(0, n, 1 << 20).astype(np.uint32)
    qd = rng.integers(0, n, 1 << 20).astype(np.uint32)
    live = np.nonzero(_live(items))[0][:1 << 19]
    qs[:len(live)], qd[:len(live)] = items[live, 0], items[live, 1]
    ts = torch.from_numpy(qs.view(np.int32)).cuda()
    td = torch.from_numpy(qd.view(np.int32)).cuda()
    tv = torch.empty(len(qs), dtype=torch.int32, device="cuda")
    e.lookup_edges_device(ts.data_ptr(), td.data_ptr(), len(qs), tv.data_ptr())
    np.testing.assert_array_equal(tv.cpu().numpy().view(np.uint32), e.lookup_edges(qs, qd))
    verts = rng.integers(0, n + 10, 1 << 18).astype(np.uint32)
    wr, wd, wv = e.gather_neighbourhoods(verts)
    tq = torch.from_numpy(verts.view(np.int32)).cuda()
    trow = torch.empty(len(verts) + 1, dtype=torch.int64, device="cuda")
    tot = e.gather_neighbourhoods_device(tq.data_ptr(), len(verts), trow.data_ptr(), 0, 0, 0)
    assert tot == len(wd)
    tdst = torch.empty(tot, dtype=torch.int32, device="cuda")
    tval = torch.empty(tot, dtype=torch.int32, device="cuda")
    assert e.gather_neighbourhoods_device(tq.data_ptr(), len(verts), trow.data_ptr(), tdst.data_ptr(), tval.data_ptr(), tot) == tot
    np.testing.assert_array_equal(trow.cpu().numpy().view(np.uint64), wr)
    np.testing.assert_array_equal(tdst.cpu().numpy(), wd)
    np.testing.assert_array_equal(tval.cpu().numpy().view(np.uint32), wv)


def test_hub_gather(pkg):
    n, hub = 1 << 16, 7
    rng = np.random.default_rng(3)
    hd = rng.choice(1 << 30, (1 << 22) + 4096, replace=False).astype(np.uint32)[:1 << 22]
    other = np.stack([rng.integers(0, n, 1 << 20), rng.integers(0, n, 1 << 20)], 1).astype(np.uint32)
    adds = np.concatenate([np.stack([np.full(len(hd), hub, np.uint32), hd], 1), other])
    adds = np.concatenate([adds, rng.integers(1, 1000, (len(adds), 1)).astype(np.uint32)], 1)
    e = pkg.PCSR(n)
    e.bulk_build(adds)
    items, nodes = e.state()
    verts = np.array([hub, 3, hub, n + 1, 12], np.uint32)
    rows, dests, vals = e.gather_neighbourhoods(verts)
    wr, wd, wv = model_gather(items, nodes, verts)
    assert int(wr[1] - wr[0]) >= 1 << 22  # (the random edges may add a few more)
    np.testing.assert_array_equal(rows, wr)
    np.testing.assert_array_equal(dests, wd)
    np.testing.assert_array_equal(vals, wv)
    got = e.lookup_edges(np.full(1 << 16, hub, np.uint32), hd[:1 << 16])
    assert np.all(got != NO_EDGE)


def test_pppcsr_p8_matches_partitions(pkg, streams):
    n, P = 1 << 18, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P, devices=[0])
    s, d = streams.rmat_edges(18, 2_000_000, seed=5)
    pp.apply(streams.adds(s, d))
    rng = np.random.default_rng(6)
    qs = np.concatenate([s[:1 << 19], rng.integers(0, n + 100, 1 << 19)]).astype(np.uint32)
    qd = np.concatenate([d[:1 << 19], rng.integers(0, n, 1 << 19)]).astype(np.uint32)
    got = pp.lookup_edges(qs, qd)
    starts = np.array([pp.partition_start(k) for k in range(P)], np.int64)
    owner = np.searchsorted(starts, qs.astype(np.int64), side="right") - 1
    parts = [pp.partition(k) for k in range(P)]
    for k in range(P):
        m = owner == k
        np.testing.assert_array_equal(got[m], parts[k].lookup_edges((qs[m] - starts[k]).astype(np.uint32), qd[m]))
    assert np.all(got[:1 << 19] != NO_EDGE)
    verts = rng.integers(0, n + 100, 1 << 18).astype(np.uint32)
    rows, dests, vals = pp.gather_neighbourhoods(verts)
    vo = np.searchsorted(starts, verts.astype(np.int64), side="right") - 1
    for k in range(P):
        m = np.nonzero(vo == k)[0]
        pr, pd, pv = parts[k].gather_neighbourhoods((verts[m] - starts[k]).astype(np.uint32))
        lens = np.diff(rows)[m]
        np.testing.assert_array_equal(lens, np.diff(pr))
        sel = np.concatenate([np.arange(int(rows[i]), int(rows[i + 1])) for i in m]) if len(m) else np.empty(0, np.int64)
        np.testing.assert_array_equal(dests[sel], pd)
        np.testing.assert_array_equal(vals[sel], pv)


def test_interleaved_batches_and_lookups(pkg, streams):
    n = 1 << 16
    e, o = pkg.PCSR(n), Oracle(n)
    rng = np.random.default_rng(8)
    for step in range(4):
        ops = streams.random_stream(n, 300_000, seed=20 + step, p_delete=0.3 if step else 0.0)
        e.apply(ops)
        o.apply(ops)
        oi, on = o.state()
        qs = np.concatenate([ops[:, 0], rng.integers(0, n, 1 << 16)]).astype(np.uint32)
        qd = np.concatenate([ops[:, 1], rng.integers(0, n, 1 << 16)]).astype(np.uint32)
        np.testing.assert_array_equal(e.lookup_edges(qs, qd), model_lookup(oi, n, qs, qd), err_msg=f"after batch {step}")
    ei, en = e.state()
    np.testing.assert_array_equal(ei, oi)
    np.testing.assert_array_equal(en, on)
