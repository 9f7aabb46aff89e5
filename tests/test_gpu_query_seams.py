"""GPU (MI355X): the batched reads across every staging, block and scan seam at the shipped sizes — host lookups over several
2^22-query round trips, gathers over several 2^20-row blocks, a gather block that gather_prepare must split because its rows
need more than 2^22 chunks, ERANGE caps at D2H window and block edges, scans of three levels (more than 4096^2 elements,
with the query_gather_* knobs raised), PPPCSR with a row larger than a whole partition stretch, and the no-write rule
around a snapshot at config #2's scale.  Answers are compared with the exact numpy models of tests/helpers.py."""
import ctypes

import numpy as np
import pytest

from helpers import (_live, check_partial_gather, digest, gather_blocks, gather_chunks, load_pkg, model_gather, model_lookup,
                     NO_EDGE)

pytestmark = pytest.mark.gpu

STAGE, ROWS, CHUNKS = 1 << 22, 1 << 20, 1 << 22  # the shipped query_lookup_stage / query_gather_stage, rows, chunks


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()
    return p


def csr_model(items, nodes, verts):
    """model_gather for in-range vertices through the whole graph's CSR: memory in the output's size, not the slots'"""
    fr, fd, fv = model_gather(items, nodes, np.arange(len(nodes), dtype=np.uint32))
    fr = fr.astype(np.int64)
    v = verts.astype(np.int64)
    lens = fr[v + 1] - fr[v]
    rows = np.concatenate([[0], np.cumsum(lens)])
    idx = np.repeat(fr[v] - rows[:-1], lens) + np.arange(int(rows[-1]), dtype=np.int64)
    return rows.astype(np.uint64), fd[idx], fv[idx]


def row_select(rows, m):
    """positions of rows m of a CSR, in order"""
    rows = rows.astype(np.int64)
    lens = rows[m + 1] - rows[m]
    cum = np.concatenate([[0], np.cumsum(lens)])
    return np.repeat(rows[m] - cum[:-1], lens) + np.arange(int(cum[-1]), dtype=np.int64)


def device_gather(e, verts, cap, with_rows=True):
    """the device form into torch tensors: (total, rows, dests, values) tensors"""
    import torch
    tq = torch.from_numpy(np.ascontiguousarray(verts).view(np.int32)).cuda()
    tr = torch.full((len(verts) + 1,), -1, dtype=torch.int64, device="cuda") if with_rows else None
    td = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    tv = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tot = ctypes.c_uint64(0)
    rc = e.L.ppcsr_gather_neighbourhoods_device(e.h, tq.data_ptr(), len(verts), tr.data_ptr() if with_rows else None, td.data_ptr(), tv.data_ptr(),
                                                cap, ctypes.byref(tot))
    assert rc in (0, 6)
    return tot.value, tr, td, tv


def device_call(e, verts):
    """check_partial_gather's call for the device form: host arrays copied to the device, gathered into, copied back"""
    import torch
    tq = torch.from_numpy(np.ascontiguousarray(verts).view(np.int32)).cuda()

    def call(r, d, v, cap, tot):
        assert cap <= len(d) and cap <= len(v)
        tr = torch.from_numpy(r.view(np.int64)).cuda()
        td = torch.from_numpy(d).cuda()
        tv = torch.from_numpy(v.view(np.int32)).cuda()
        torch.cuda.synchronize()
        rc = e.L.ppcsr_gather_neighbourhoods_device(e.h, tq.data_ptr(), len(verts), tr.data_ptr(), td.data_ptr(), tv.data_ptr(), cap, ctypes.byref(tot))
        torch.cuda.synchronize()
        r[:] = tr.cpu().numpy().view(np.uint64)
        d[:] = td.cpu().numpy()
        v[:] = tv.cpu().numpy().view(np.uint32)
        return rc
    return call


def host_call(e, verts):
    q = np.ascontiguousarray(verts)

    def call(r, d, v, cap, tot):
        return e.L.ppcsr_gather_neighbourhoods(e.h, q.ctypes.data, len(q), r.ctypes.data, d.ctypes.data, v.ctypes.data, cap, ctypes.byref(tot))
    return call


def same_on_device(t, a, label, step=1 << 24):
    """device tensor t equals host array a, compared slice by slice on the device"""
    import torch
    assert t.numel() >= len(a), label
    for i in range(0, len(a), step):
        h = torch.from_numpy(np.ascontiguousarray(a[i:i + step])).cuda()
        assert torch.equal(t[i:i + len(h)], h), f"{label}: differs in [{i}, {i + len(h)})"


@pytest.fixture(scope="module")
def rmat(pkg, streams):
    """RMAT scale 20, 4 M edges, bulk-built"""
    n = 1 << 20
    s, d = streams.rmat_edges(20, 4_000_000, seed=11)
    e = pkg.PCSR(n)
    e.bulk_build(np.stack([s, d, (np.arange(len(s)) % 1000 + 1).astype(np.uint32)], 1))
    items, nodes = e.state()
    return e, items, nodes


@pytest.fixture(scope="module")
def hubg(pkg):
    """2^16 vertices, 2^20 random edges and a hub of 2^22 edges at vertex 7 (the test_hub_gather graph)"""
    n, hub = 1 << 16, 7
    rng = np.random.default_rng(3)
    hd = rng.choice(1 << 30, (1 << 22) + 4096, replace=False).astype(np.uint32)[:1 << 22]
    other = np.stack([rng.integers(0, n, 1 << 20), rng.integers(0, n, 1 << 20)], 1).astype(np.uint32)
    adds = np.concatenate([np.stack([np.full(len(hd), hub, np.uint32), hd], 1), other])
    adds = np.concatenate([adds, rng.integers(1, 1000, (len(adds), 1)).astype(np.uint32)], 1)
    e = pkg.PCSR(n)
    e.bulk_build(adds)
    items, nodes = e.state()
    return e, items, nodes, hub


# ---- a. lookup stages ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [STAGE + 1, 2 * STAGE + 12345])
def test_lookup_stages(rmat, nq):
    import torch
    e, items, nodes = rmat
    n = len(nodes)
    rng = np.random.default_rng(nq)
    live = np.nonzero(_live(items))[0]
    qs = rng.integers(0, n + 1000, nq).astype(np.uint32)
    qd = rng.integers(0, n, nq).astype(np.uint32)
    half = rng.random(nq) < 0.5
    pick = live[rng.integers(0, len(live), int(half.sum()))]
    qs[half], qd[half] = items[pick, 0], items[pick, 1]
    for j in range(1, nq // STAGE + 1):  # known edges on both sides of every stage edge
        for i in (j * STAGE - 1, j * STAGE, j * STAGE + 1):
            if i < nq:
                qs[i], qd[i] = items[live[i % len(live)], :2]
    qs[-1], qd[-1] = items[live[-1], :2]
    got = e.lookup_edges(qs, qd)
    want = model_lookup(items, n, qs, qd)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} lookups differ, first at {bad[:8]}"
    for j in range(1, nq // STAGE + 1):
        assert np.all(got[j * STAGE - 1:j * STAGE + 2] != NO_EDGE)
    ts, td = torch.from_numpy(qs.view(np.int32)).cuda(), torch.from_numpy(qd.view(np.int32)).cuda()
    tv = torch.full((nq + 16,), -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.lookup_edges_device(ts.data_ptr(), td.data_ptr(), nq, tv.data_ptr())
    same_on_device(tv[:nq], got.view(np.int32), "device lookups")
    assert bool((tv[nq:] == -3).all())


# ---- b. row blocks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [ROWS + 1, 2 * ROWS + 7])
def test_gather_row_blocks(rmat, k):
    e, items, nodes = rmat
    n = len(nodes)
    rng = np.random.default_rng(k)
    verts = rng.integers(0, n + 100, k).astype(np.uint32)
    rows, dests, vals = e.gather_neighbourhoods(verts)
    wr, wd, wv = model_gather(items, nodes, verts)
    for i0 in range(ROWS, k, ROWS):
        np.testing.assert_array_equal(rows[i0 - 2:i0 + 3], wr[i0 - 2:i0 + 3], err_msg=f"row offsets around {i0}")
    np.testing.assert_array_equal(rows, wr)
    np.testing.assert_array_equal(dests, wd)
    np.testing.assert_array_equal(vals, wv)
    tot, tr, td, tv = device_gather(e, verts, len(wd))
    assert tot == len(wd)
    same_on_device(tr, wr.view(np.int64), "device row offsets")
    same_on_device(td, wd, "device dests")
    same_on_device(tv, wv.view(np.int32), "device values")


# ---- c. the chunk split inside a block ---------------------------------------------------------------------------------------
def test_gather_chunk_split_shipped(hubg):
    """44 hub rows interleaved with small rows, all in one block of rows: more than 2^22 chunks, so gather_prepare splits the
    block at row boundaries that are not block boundaries.  Hub slices against the hub's own gather, small rows against the
    model, the device form against the host form on the device"""
    import torch
    e, items, nodes, hub = hubg
    n = len(nodes)
    rng = np.random.default_rng(50)
    small = rng.integers(0, n + 10, (44, 60)).astype(np.uint32)
    small[small == hub] = 8
    verts = np.ascontiguousarray(np.concatenate([np.concatenate([[hub], s]) for s in small]).astype(np.uint32))
    nch = gather_chunks(nodes, verts)
    assert len(verts) < ROWS and nch.sum() > CHUNKS  # (the split runs)
    blocks = gather_blocks(nodes, verts, ROWS, CHUNKS)
    assert len(blocks) >= 3
    _, hd, hv = e.gather_neighbourhoods(np.array([hub], np.uint32))
    H = len(hd)
    assert H >= 1 << 22
    rows, dests, vals = e.gather_neighbourhoods(verts)
    hi = np.nonzero(verts == hub)[0]
    si = np.nonzero(verts != hub)[0]
    lens = np.diff(rows.astype(np.int64))
    assert np.all(lens[hi] == H)
    sr, sd, sv = model_gather(items, nodes, verts[si])
    np.testing.assert_array_equal(lens[si], np.diff(sr.astype(np.int64)))
    assert int(rows[-1]) == len(dests) == 44 * H + len(sd)
    for i in hi:
        a = int(rows[i])
        assert np.array_equal(dests[a:a + H], hd) and np.array_equal(vals[a:a + H], hv), f"hub row {i}"
    sel = row_select(rows, si)
    np.testing.assert_array_equal(dests[sel], sd)
    np.testing.assert_array_equal(vals[sel], sv)
    del sel
    tot, tr, td, tv = device_gather(e, verts, len(dests))
    assert tot == len(dests)
    same_on_device(tr, rows.view(np.int64), "device row offsets")
    same_on_device(td, dests, "device dests")
    same_on_device(tv, vals.view(np.int32), "device values")
    del td, tv
    torch.cuda.empty_cache()


def test_gather_chunk_split_many_times(pkg, streams):
    """query_gather_chunks = 2^16 on a smaller graph with a hub of 2^22 edges: every block is split many times, and the hub's
    row (about 10^5 chunks) is a block of its own; full model"""
    n = 1 << 18
    s, d = streams.rmat_edges(18, 2_000_000, seed=12)
    hub = np.stack([np.full(1 << 22, 77, np.uint32), np.arange(1 << 22, dtype=np.uint32) * 3 + 1], 1)
    adds = np.concatenate([np.stack([s, d], 1), hub])
    adds = np.concatenate([adds, (np.arange(len(adds)) % 997 + 1).astype(np.uint32)[:, None]], 1)
    e = pkg.PCSR(n)
    e.bulk_build(adds)
    items, nodes = e.state()
    rng = np.random.default_rng(51)
    verts = rng.integers(0, n + 10, (1 << 20) + 5).astype(np.uint32)
    verts[[1000, 1001, 600_000]] = 77
    e.set_option("query_gather_chunks", 1 << 16)
    blocks = gather_blocks(nodes, verts, ROWS, 1 << 16)
    assert len(blocks) - 1 > 10
    assert any(gather_chunks(nodes, verts)[blocks[:-1]] > 1 << 16)  # (a hub row is a block of its own)
    wr, wd, wv = model_gather(items, nodes, verts)
    rows, dests, vals = e.gather_neighbourhoods(verts)
    np.testing.assert_array_equal(rows, wr)
    np.testing.assert_array_equal(dests, wd)
    np.testing.assert_array_equal(vals, wv)
    tot, tr, td, tv = device_gather(e, verts, len(wd))
    assert tot == len(wd)
    same_on_device(tr, wr.view(np.int64), "device row offsets")
    same_on_device(td, wd, "device dests")
    same_on_device(tv, wv.view(np.int32), "device values")
    e.set_option("query_gather_chunks", CHUNKS)


# ---- d. windows and ERANGE -----------------------------------------------------------------------------------------------------
def test_gather_windows_and_erange(hubg):
    """more than 2^22 output edges with the window edge 2^22 inside the hub's row, and a block edge at row 2^20"""
    e, items, nodes, hub = hubg
    n = len(nodes)
    rng = np.random.default_rng(52)
    deg = np.diff(model_gather(items, nodes, np.arange(n, dtype=np.uint32))[0].astype(np.int64))
    pre = int(((1 << 22) - (1 << 21)) // max(deg.mean(), 1))
    verts = rng.integers(0, n, ROWS + 101).astype(np.uint32)
    verts[verts == hub] = 8
    verts[pre] = hub
    want = csr_model(items, nodes, verts)
    wr = want[0].astype(np.int64)
    T = int(wr[-1])
    assert wr[pre] < (1 << 22) < wr[pre + 1] and T > 2 * (1 << 22)
    b = int(wr[ROWS])
    caps = sorted({(1 << 22) - 1, 1 << 22, (1 << 22) + 1, b - 1, b, b + 1, T - 1, T, 2 * (1 << 22) + 1})
    for cap in caps:
        check_partial_gather(host_call(e, verts), *want, cap)
    for cap in caps:
        check_partial_gather(device_call(e, verts), *want, cap)


# ---- e. three-level scans --------------------------------------------------------------------------------------------------------
def test_gather_three_level_scans(pkg):
    """4096 * 4096 + 4097 rows in one block (query_gather_rows = 2^25, query_gather_chunks = 2^26): the row-chunk scan, the
    chunk -> row max-scan and the output scan recurse three levels; against the model and the default-knob (16-block) gather"""
    import threading
    import time
    peak, done = [0], threading.Event()

    def sample():  # host memory of this test: the largest resident set seen while it runs (ru_maxrss spans the whole session)
        while not done.is_set():
            with open("/proc/self/status") as f:
                peak[0] = max(peak[0], next(int(l.split()[1]) for l in f if l.startswith("VmRSS")))
            time.sleep(0.02)
    th = threading.Thread(target=sample, daemon=True)
    th.start()
    n = 1 << 20
    rng = np.random.default_rng(53)
    adds = np.stack([rng.integers(0, n, 1 << 21), rng.integers(0, n, 1 << 21), rng.integers(1, 1 << 30, 1 << 21)], 1).astype(np.uint32)
    e = pkg.PCSR(n)
    e.bulk_build(adds)
    items, nodes = e.state()
    k = 4096 * 4096 + 4097
    ne = np.nonzero(gather_chunks(nodes, np.arange(n, dtype=np.uint32)) > 0)[0].astype(np.uint32)
    verts = ne[rng.integers(0, len(ne), k)]
    assert gather_chunks(nodes, verts).sum() > 4096 * 4096
    del items
    want = csr_model(*e.state(), verts)
    e.set_option("query_gather_rows", 1 << 25)
    e.set_option("query_gather_chunks", 1 << 26)
    rows, dests, vals = e.gather_neighbourhoods(verts)
    assert len(dests) > 4096 * 4096
    np.testing.assert_array_equal(rows, want[0])
    np.testing.assert_array_equal(dests, want[1])
    np.testing.assert_array_equal(vals, want[2])
    tot, tr, td, tv = device_gather(e, verts, len(want[1]))
    assert tot == len(want[1])
    same_on_device(tr, want[0].view(np.int64), "device row offsets")
    same_on_device(td, want[1], "device dests")
    same_on_device(tv, want[2].view(np.int32), "device values")
    del tr, td, tv
    e.set_option("query_gather_rows", ROWS)
    e.set_option("query_gather_chunks", CHUNKS)
    r2, d2, v2 = e.gather_neighbourhoods(verts)
    np.testing.assert_array_equal(r2, rows)
    np.testing.assert_array_equal(d2, dests)
    np.testing.assert_array_equal(v2, vals)
    done.set()
    th.join()
    print(f"\nthree-level scans: peak resident set {peak[0] / 1024:.0f} MiB during the test")


# ---- f. PPPCSR, P = 8 on one GPU ------------------------------------------------------------------------------------------------
def check_pp(pp, rng, label):
    P = pp.num_partitions()
    N = pp.get_n()
    starts = np.array([pp.partition_start(k) for k in range(P)], np.int64)
    parts = [pp.partition(k) for k in range(P)]
    states = [p.state() for p in parts]
    hub = 3 * (1 << 17) + 5
    for nq in ((1 << 20) + 1, 3 * (1 << 20) + 5):
        qs = rng.integers(0, N + 100, nq).astype(np.uint32)
        qd = rng.integers(0, N, nq).astype(np.uint32)
        got = pp.lookup_edges(qs, qd)
        own = np.searchsorted(starts, qs.astype(np.int64), side="right") - 1
        for k in range(P):
            m = own == k
            lq = (qs[m] - np.uint32(starts[k])).astype(np.uint32)
            np.testing.assert_array_equal(got[m], parts[k].lookup_edges(lq, qd[m]), err_msg=f"{label}: lookups, partition {k}")
            np.testing.assert_array_equal(got[m], model_lookup(states[k][0], len(states[k][1]), lq, qd[m]), err_msg=f"{label}: lookup model {k}")
    verts = rng.integers(0, N + 100, (1 << 20) + 3).astype(np.uint32)
    verts[[5, 6, (1 << 20) - 2, (1 << 20) + 1]] = hub
    rows, dests, vals = pp.gather_neighbourhoods(verts)
    own = np.searchsorted(starts, verts.astype(np.int64), side="right") - 1
    hk = int(np.searchsorted(starts, hub, side="right") - 1)
    assert int(np.diff(rows.astype(np.int64))[5]) > 1 << 22  # (a row larger than a partition stretch)
    for k in range(P):
        m = np.nonzero(own == k)[0]
        lv = (verts[m] - np.uint32(starts[k])).astype(np.uint32)
        pr, pd, pv = parts[k].gather_neighbourhoods(lv)
        if k == hk:
            assert int(pr[-1]) > 1 << 22
        mr, md, mv = model_gather(states[k][0], states[k][1], lv)
        np.testing.assert_array_equal(pr, mr, err_msg=f"{label}: partition {k} model")
        np.testing.assert_array_equal(np.diff(rows.astype(np.int64))[m], np.diff(pr.astype(np.int64)), err_msg=f"{label}: rows {k}")
        sel = row_select(rows, m)
        np.testing.assert_array_equal(dests[sel], pd, err_msg=f"{label}: dests {k}")
        np.testing.assert_array_equal(vals[sel], pv, err_msg=f"{label}: values {k}")
        np.testing.assert_array_equal(pd, md)
        np.testing.assert_array_equal(pv, mv)


def test_pppcsr_p8_seams(pkg, streams):
    import torch
    n, P = 1 << 20, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P, devices=[0])
    s, d = streams.rmat_edges(20, 2_000_000, seed=54)
    hub = 3 * (1 << 17) + 5
    hd = np.arange((1 << 22) + 1000, dtype=np.uint32) * 3 + 1
    adds = np.concatenate([np.stack([s, d], 1), np.stack([np.full(len(hd), hub, np.uint32), hd], 1)])
    adds = np.concatenate([adds, (np.arange(len(adds)) % 991 + 1).astype(np.uint32)[:, None]], 1)
    t = torch.from_numpy(np.ascontiguousarray(adds).view(np.int32)).cuda()
    torch.cuda.synchronize()
    pp.bulk_build_device(t.data_ptr(), len(adds))
    del t
    rng = np.random.default_rng(55)
    check_pp(pp, rng, "default layout")
    pp.repartition(pp.balanced_starts())
    check_pp(pp, rng, "balanced layout")


# ---- g. nothing is written, around a snapshot -----------------------------------------------------------------------------------
def test_queries_write_nothing_config2(pkg, streams):
    import torch
    n = 1 << 20
    s, d = streams.rmat_edges(20, 10_000_000, seed=1)
    core = streams.adds(s, d)
    e = pkg.PCSR(n)
    e.apply(core)
    e.snapshot()
    d0 = digest(*e.state(), e.geometry())
    s2, d2 = streams.rmat_edges(20, 1_000_000, seed=2)
    e.apply(streams.mixed_existing_stream(core, streams.adds(s2, d2)[:500_000], seed=3))
    st, geom = e.stats(), e.geometry()
    items, nodes = e.state()
    d1 = digest(items, nodes, geom)
    assert d1 != d0
    rng = np.random.default_rng(56)
    qs = rng.integers(0, n + 10, STAGE + 1).astype(np.uint32)
    qd = rng.integers(0, n, STAGE + 1).astype(np.uint32)
    e.lookup_edges(qs, qd)
    ts, td = torch.from_numpy(qs.view(np.int32)).cuda(), torch.from_numpy(qd.view(np.int32)).cuda()
    tv = torch.empty(len(qs), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.lookup_edges_device(ts.data_ptr(), td.data_ptr(), len(qs), tv.data_ptr())
    verts = rng.integers(0, n + 10, ROWS + 1).astype(np.uint32)
    rows, dests, vals = e.gather_neighbourhoods(verts)
    tot, tr, tdd, tvv = device_gather(e, verts, len(dests))
    assert tot == len(dests)
    check_partial_gather(host_call(e, verts), rows, dests, vals, len(dests) // 2)
    assert e.stats() == st and e.geometry() == geom
    assert digest(*e.state(), e.geometry()) == d1
    e.restore()
    assert digest(*e.state(), e.geometry()) == d0
