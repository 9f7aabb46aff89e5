"""CPU: the seams of the batched reads on the fiber SIMT emulator (tests/hostsim).  The host code splits every call into
pieces — lookups per staging round trip, gather rows per block, chunks per block (the split inside gather_prepare), output
edges per D2H window, PPPCSR queries per routed block and edges per partition stretch — and the shipped sizes are far beyond
what the emulator can reach.  The "query_*" knobs of ppcsr_set_option and pppcsr_set_option shrink them here, so every seam
is crossed many times, with hubs that span many 64-slot chunks and rows that are larger than a whole block.  Answers are
compared with the exact numpy models of tests/helpers.py (model_lookup / model_gather on the exported state) and with the
default-knob answer; partial gathers with check_partial_gather.  The states are built once per module: queries write
nothing (checked by test_sim_queries_write_nothing)."""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import (ERANGE, NO_EDGE, _live, check_partial_gather, gather_blocks, gather_chunks, load_pkg, model_gather,
                     model_lookup)
from test_sim_engine import SIM_SO, build_sim
from test_sim_queries import make

DEFAULTS = {"query_lookup_stage": 1 << 22, "query_gather_rows": 1 << 20, "query_gather_chunks": 1 << 22, "query_gather_stage": 1 << 22}
HUB = 5


@pytest.fixture(scope="module")
def lib():
    build_sim()
    L = load_pkg().load_library(SIM_SO)
    L.ppcsr_sim_fail_alloc_after.argtypes = [ctypes.c_int]
    return L


def knobs(e, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        e.set_option(k, v)


def hub_graph(streams):
    """the test_sim_gather_multi_tile_scans shape: random edges over 3000 vertices and a hub of 2500 edges at HUB"""
    n = 3000
    hub = np.stack([np.full(2500, HUB, np.uint32), np.arange(2500, dtype=np.uint32) * 3 + 1, np.arange(2500, dtype=np.uint32) + 2], 1)
    return n, np.concatenate([streams.random_stream(n, 12000, seed=12), hub])


def sparse_graph(streams):
    """edges from every third vertex only, a hub at the LAST vertex (its range ends at slot N - 1), then every edge of the
    multiples of 9 deleted: vertices with empty ranges, ranges of null slots only, and live rows between them"""
    n = 2000
    ops = streams.random_stream(n, 6000, seed=31)
    ops = ops[ops[:, 0] % 3 == 0]
    hub = np.stack([np.full(700, n - 1, np.uint32), np.arange(700, dtype=np.uint32) * 7 + 3, np.arange(700, dtype=np.uint32) + 1], 1)
    dele = ops[ops[:, 0] % 9 == 0].copy()
    dele[:, 2] = 0
    return n, np.concatenate([ops, hub, dele])


@pytest.fixture(scope="module")
def graphs(lib, streams):
    out = {}
    for name, (n, ops), hub in (("hub", hub_graph(streams), HUB), ("sparse", sparse_graph(streams), 1999)):
        e = make(lib, n)
        e.apply(ops)
        items, nodes = e.state()
        out[name] = (e, items, nodes, hub)
    return out


def lookup_queries(rng, items, nodes, hub, m=600):
    """present pairs, random pairs, src >= n and 0xFFFFFFFF, dst 0 and 0xFFFFFFFF, repeats, and a run of the hub's edges"""
    n = len(nodes)
    live = np.nonzero(_live(items))[0]
    present = items[live[rng.integers(0, len(live), m // 3)], :2]
    parts = [present,
             np.stack([rng.integers(0, n, m // 6), rng.integers(0, 2 * n, m // 6)], 1),
             np.stack([rng.integers(n, n + 100, 20), rng.integers(0, n, 20)], 1),
             np.array([[n, 0], [0xFFFFFFFF, 0], [0xFFFFFFFF, 0xFFFFFFFF], [0, 0xFFFFFFFF], [hub, 0xFFFFFFFF], [hub, 0]]),
             np.stack([rng.integers(0, n, 20), np.zeros(20, np.int64)], 1),
             np.stack([rng.integers(0, n, 20), np.full(20, 0xFFFFFFFF)], 1)]
    q = np.concatenate([p.astype(np.uint32) for p in parts])
    q = np.concatenate([q, q[rng.integers(0, len(q), m // 10)]])
    q = q[rng.permutation(len(q))]
    hl = live[items[live, 0] == hub]
    run = np.concatenate([items[hl[:60], :2], np.stack([np.full(10, hub), rng.integers(0, 1 << 20, 10)], 1).astype(np.uint32)])
    q = np.concatenate([q[:len(q) // 2], run, q[len(q) // 2:]])
    return np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])


def gather_queries(rng, nodes, hub, k=260, run=3):
    """random vertices with repeats, out-of-range ones, the hub `run` times in a row and once more on its own"""
    n = len(nodes)
    v = np.concatenate([rng.integers(0, n, k), [n, n + 3, 0xFFFFFFFF, 0]]).astype(np.uint32)
    v = v[rng.permutation(len(v))]
    return np.ascontiguousarray(np.concatenate([v[:k // 3], np.full(run, hub, np.uint32), v[k // 3:2 * k // 3], [hub], v[2 * k // 3:]]).astype(np.uint32))


def gather_host(e, verts, rows=True, dests=True, values=True, cap=None):
    """the raw host call: (rc, total, rows | None, dests | None, values | None)"""
    q = np.ascontiguousarray(verts, np.uint32)
    tot = ctypes.c_uint64(0)
    if cap is None:
        assert e.L.ppcsr_gather_neighbourhoods(e.h, q.ctypes.data, len(q), None, None, None, 0, ctypes.byref(tot)) == 0
        cap = tot.value
    r = np.full(len(q) + 1, 0xDEAD, np.uint64) if rows else None
    d = np.full(cap + 4, -7, np.int32) if dests else None
    v = np.full(cap + 4, 0xA5A5A5A5, np.uint32) if values else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = e.L.ppcsr_gather_neighbourhoods(e.h, q.ctypes.data, len(q), ptr(r), ptr(d), ptr(v), cap, ctypes.byref(tot))
    return rc, tot.value, r, d, v


def gather_device(e, verts, rows=True, dests=True, values=True, cap=None):
    """the device form through its raw C call (on the emulator a device allocation is malloc: host arrays stand in for HBM)"""
    q = np.ascontiguousarray(verts, np.uint32)
    tot = ctypes.c_uint64(0)
    if cap is None:
        assert e.L.ppcsr_gather_neighbourhoods_device(e.h, q.ctypes.data, len(q), None, None, None, 0, ctypes.byref(tot)) == 0
        cap = tot.value
    r = np.full(len(q) + 1, 0xDEAD, np.uint64) if rows else None
    d = np.full(cap + 4, -7, np.int32) if dests else None
    v = np.full(cap + 4, 0xA5A5A5A5, np.uint32) if values else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = e.L.ppcsr_gather_neighbourhoods_device(e.h, q.ctypes.data, len(q), ptr(r), ptr(d), ptr(v), cap, ctypes.byref(tot))
    return rc, tot.value, r, d, v


def full(form, e, verts, want, **kw):
    return form(e, verts, cap=len(want[1]), **kw)


def check_full(got, want, label):
    rc, tot, r, d, v = got
    wr, wd, wv = want
    T = len(wd)
    assert rc == 0 and tot == T, (label, rc, tot, T)
    if r is not None:
        np.testing.assert_array_equal(r, wr, err_msg=label + ": row offsets")
    if d is not None:
        np.testing.assert_array_equal(d[:T], wd, err_msg=label + ": dests")
        assert np.all(d[T:] == -7), label
    if v is not None:
        np.testing.assert_array_equal(v[:T], wv, err_msg=label + ": values")
        assert np.all(v[T:] == 0xA5A5A5A5), label


# ---- the knobs ---------------------------------------------------------------------------------------------------------
def test_sim_query_knobs_validated(lib):
    pkg = load_pkg()
    e = make(lib, 10)
    for key in DEFAULTS:
        for bad in (0, -1, -(1 << 40), (1 << 32) + 1):
            with pytest.raises(pkg.PpcsrError):
                e.set_option(key, bad)
        e.set_option(key, 1)
        e.set_option(key, 1 << 26)
    pp = pkg.PPPCSR(40, numDomain=1, partitionsPerDomain=2, lib=lib)
    for key in ("query_block", "gather_stage"):
        for bad in (0, -1, (1 << 32) + 1):
            assert lib.pppcsr_set_option(pp.h, key.encode(), bad) == 1
        pp.set_option(key, 1)
        pp.set_option(key, 1 << 26)
    assert lib.pppcsr_set_option(pp.h, b"query_lookup_stage", 5) == 1  # (an engine key is not a PPPCSR key)
    assert lib.pppcsr_set_option(None, b"query_block", 5) == 1


def test_sim_knobs_lowered_then_raised(graphs):
    """every knob at 1, then far above the defaults, then back: the scratch each call needs is regrown as it grows; unset
    knobs (a fresh handle's defaults) and the defaults set explicitly answer alike"""
    e, items, nodes, hub = graphs["hub"]
    rng = np.random.default_rng(40)
    qs, qd = lookup_queries(rng, items, nodes, hub, m=300)
    verts = gather_queries(rng, nodes, hub, k=100, run=1)
    wl, wg = model_lookup(items, len(nodes), qs, qd), model_gather(items, nodes, verts)
    base = (e.lookup_edges(qs, qd), e.gather_neighbourhoods(verts))
    low = {k: 1 for k in DEFAULTS}
    low["query_gather_stage"] = 7
    for label, kw in (("low", low), ("2^26", {k: 1 << 26 for k in DEFAULTS}), ("low again", low), ("defaults", DEFAULTS)):
        knobs(e, **kw)
        np.testing.assert_array_equal(e.lookup_edges(qs, qd), wl, err_msg=label)
        check_full(full(gather_host, e, verts, wg), wg, "host, knobs " + label)
        check_full(full(gather_device, e, verts, wg), wg, "device, knobs " + label)
    np.testing.assert_array_equal(base[0], wl)
    for a, b in zip(base[1], wg):
        np.testing.assert_array_equal(a, b)


# ---- lookups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "sparse"])
def test_sim_lookup_stages(graphs, graph):
    e, items, nodes, hub = graphs[graph]
    n = len(nodes)
    qs, qd = lookup_queries(np.random.default_rng(41), items, nodes, hub)
    want = model_lookup(items, n, qs, qd)
    assert np.mean(want != NO_EDGE) > 0.3 and len(qs) > 100
    knobs(e)
    np.testing.assert_array_equal(e.lookup_edges(qs, qd), want, err_msg="default stage")
    for stage in (1, 63, 64, 65, 100):
        knobs(e, query_lookup_stage=stage)
        np.testing.assert_array_equal(e.lookup_edges(qs, qd), want, err_msg=f"stage {stage}")
        np.testing.assert_array_equal(e.lookup_edges(qs[:stage + 1], qd[:stage + 1]), want[:stage + 1], err_msg=f"stage {stage} + 1")
    knobs(e)
    out = np.full(len(qs) + 3, 0x5A5A5A5A, np.uint32)
    assert e.L.ppcsr_lookup_edges_device(e.h, qs.ctypes.data, qd.ctypes.data, len(qs), out.ctypes.data) == 0
    np.testing.assert_array_equal(out[:len(qs)], want, err_msg="device form")
    assert np.all(out[len(qs):] == 0x5A5A5A5A)


# ---- gathers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "sparse"])
@pytest.mark.parametrize("rows,chunks", list(itertools.product((1, 2, 7), (1, 5, 64))))
def test_sim_gather_blocks_and_windows(graphs, graph, rows, chunks):
    e, items, nodes, hub = graphs[graph]
    verts = gather_queries(np.random.default_rng(42), nodes, hub)
    want = model_gather(items, nodes, verts)
    nch = gather_chunks(nodes, verts)
    blocks = gather_blocks(nodes, verts, rows, chunks)
    assert nch[list(verts).index(hub)] > 5  # (the hub spans several chunks)
    if chunks < 64:  # the split in gather_prepare, and rows larger than a whole block
        assert len(blocks) - 1 > -(-len(verts) // rows) or rows == 1
        assert any(nch[blocks[j]] > chunks for j in range(len(blocks) - 1))
    for stage in (33, 64):
        knobs(e, query_gather_rows=rows, query_gather_chunks=chunks, query_gather_stage=stage)
        check_full(full(gather_host, e, verts, want), want, f"host, stage {stage}")
    # one D2H round trip per edge: on the rows without the hub (the emulator launches a kernel per window)
    few = np.ascontiguousarray(verts[verts != hub][:90])
    knobs(e, query_gather_rows=rows, query_gather_chunks=chunks, query_gather_stage=1)
    check_full(gather_host(e, few), model_gather(items, nodes, few), "host, stage 1")
    check_full(full(gather_device, e, verts, want), want, "device")
    # the optional outputs: no row offsets, no dests, only the size
    knobs(e, query_gather_rows=rows, query_gather_chunks=chunks, query_gather_stage=33)
    for form in (gather_host, gather_device):
        check_full(full(form, e, verts, want, rows=False), want, f"{form.__name__}, row_offsets NULL")
        check_full(full(form, e, verts, want, dests=False), want, f"{form.__name__}, dests NULL")
        check_full(form(e, verts, dests=False, values=False), want, f"{form.__name__}, size query")
        check_full(form(e, verts, rows=False, dests=False, values=False), want, f"{form.__name__}, total only")
    knobs(e)


def erange_caps(want, verts, nodes, hub, rows, chunks, stage, rng):
    """0, 1, total - 1, total, block edges and window edges +- 1 (a sample of them), caps inside the hub's row"""
    wr = want[0].astype(np.int64)
    T = int(wr[-1])
    blocks = gather_blocks(nodes, verts, rows, chunks)
    bedge = wr[blocks]
    wedge = np.concatenate([np.arange(int(bedge[j]) + stage, int(bedge[j + 1]), stage) for j in range(len(blocks) - 1)] + [np.empty(0, np.int64)])
    pick = lambda a, m: a[rng.choice(len(a), min(m, len(a)), replace=False)] if len(a) else a
    i = list(verts).index(hub)
    caps = {0, 1, T - 1, T, int(wr[i]) + 1, (int(wr[i]) + int(wr[i + 1])) // 2, int(wr[i + 1]) - 1}
    for x in np.concatenate([pick(bedge[1:-1], 5), pick(wedge, 5)]):
        caps |= {int(x) - 1, int(x), int(x) + 1}
    return sorted(c for c in caps if 0 <= c <= T)


@pytest.mark.parametrize("rows,chunks,stage", [(7, 64, 33), (2, 5, 17)])
def test_sim_gather_erange(graphs, rows, chunks, stage):
    e, items, nodes, hub = graphs["hub"]
    rng = np.random.default_rng(43)
    verts = gather_queries(rng, nodes, hub, k=120, run=1)
    want = model_gather(items, nodes, verts)
    q = np.ascontiguousarray(verts)
    knobs(e, query_gather_rows=rows, query_gather_chunks=chunks, query_gather_stage=stage)

    def host(r, d, v, cap, tot):
        return e.L.ppcsr_gather_neighbourhoods(e.h, q.ctypes.data, len(q), r.ctypes.data, d.ctypes.data, v.ctypes.data, cap, ctypes.byref(tot))

    def device(r, d, v, cap, tot):
        return e.L.ppcsr_gather_neighbourhoods_device(e.h, q.ctypes.data, len(q), r.ctypes.data, d.ctypes.data, v.ctypes.data, cap,
                                                      ctypes.byref(tot))

    caps = erange_caps(want, verts, nodes, hub, rows, chunks, stage, rng)
    assert len(caps) > 20
    for cap in caps:
        check_partial_gather(host, *want, cap)
        check_partial_gather(device, *want, cap)
    # dests only / values only past the cap
    cap = caps[len(caps) // 2]
    for form in (gather_host, gather_device):
        rc, tot, r, d, v = form(e, verts, values=False, cap=cap)
        assert rc == ERANGE and tot == len(want[1])
        np.testing.assert_array_equal(d[:cap], want[1][:cap])
        assert np.all(d[cap:] == -7)
        rc, tot, r, d, v = form(e, verts, dests=False, cap=cap)
        assert rc == ERANGE and tot == len(want[1])
        np.testing.assert_array_equal(v[:cap], want[2][:cap])
        assert np.all(v[cap:] == 0xA5A5A5A5)
    knobs(e)


# ---- PPPCSR --------------------------------------------------------------------------------------------------------------
def pp_model(pp, qs, qd, verts):
    """the answers of the partition states' models, in the caller's order"""
    P = pp.num_partitions()
    starts = np.array([pp.partition_start(k) for k in range(P)], np.int64)
    st = [pp.partition(k).state() for k in range(P)]
    own = np.searchsorted(starts, qs.astype(np.int64), side="right") - 1
    vals = np.empty(len(qs), np.uint32)
    for k in range(P):
        m = own == k
        vals[m] = model_lookup(st[k][0], len(st[k][1]), (qs[m] - np.uint32(starts[k])).astype(np.uint32), qd[m])
    own = np.searchsorted(starts, verts.astype(np.int64), side="right") - 1
    rows, dests, gv = [0], [], []
    for i, v in enumerate(verts):
        k = own[i]
        _, d, w = model_gather(st[k][0], st[k][1], np.array([int(v) - starts[k]], np.uint32))
        rows.append(rows[-1] + len(d))
        dests.append(d)
        gv.append(w)
    return vals, (np.array(rows, np.uint64), np.concatenate(dests), np.concatenate(gv))


def pp_per_partition(pp, qs, qd, verts):
    """the same questions asked of every partition with the single-engine calls"""
    P = pp.num_partitions()
    starts = np.array([pp.partition_start(k) for k in range(P)], np.int64)
    parts = [pp.partition(k) for k in range(P)]
    own = np.searchsorted(starts, qs.astype(np.int64), side="right") - 1
    vals = np.empty(len(qs), np.uint32)
    for k in range(P):
        m = own == k
        if m.any():
            vals[m] = parts[k].lookup_edges((qs[m] - np.uint32(starts[k])).astype(np.uint32), qd[m])
    own = np.searchsorted(starts, verts.astype(np.int64), side="right") - 1
    lens = np.zeros(len(verts), np.int64)
    dl, vl = [None] * len(verts), [None] * len(verts)
    for k in range(P):
        m = np.nonzero(own == k)[0]
        if len(m) == 0:
            continue
        r, d, w = parts[k].gather_neighbourhoods((verts[m] - np.uint32(starts[k])).astype(np.uint32))
        for j, i in enumerate(m):
            dl[i], vl[i] = d[int(r[j]):int(r[j + 1])], w[int(r[j]):int(r[j + 1])]
            lens[i] = len(dl[i])
    return vals, (np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), np.concatenate(dl), np.concatenate(vl))


def test_sim_pppcsr_blocks_and_stretches(lib, streams):
    """P = 4: query_block in {1, 13} x gather_stage in {1, 17} against per-partition calls and the partition models, on the
    default layout, after a repartition to unequal starts with one empty partition, and after add_node on the last one"""
    pkg = load_pkg()
    n, P = 400, 4
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P, lib=lib)
    hub = np.stack([np.full(400, 250, np.uint32), np.arange(400, dtype=np.uint32) * 5 + 1, np.arange(400, dtype=np.uint32) + 1], 1)
    pp.apply(np.concatenate([streams.random_stream(n, 3000, seed=9, p_delete=0.2), hub]))
    rng = np.random.default_rng(44)
    layouts = [("default", None), ("[0, 50, 50, 299]", np.array([0, 50, 50, 299], np.uint64)), ("add_node x3", "add_node")]
    for label, lay in layouts:
        if isinstance(lay, np.ndarray):
            pp.repartition(lay)
            assert [pp.partition_start(k) for k in range(P)] == [int(x) for x in lay]
        elif lay == "add_node":
            for _ in range(3):
                pp.add_node()
        N = pp.get_n()
        items = np.concatenate([pp.partition(k).state()[0] for k in range(P)])
        live = items[_live(items)]
        qs = np.concatenate([rng.integers(0, N, 150), np.full(30, 250), [N, N + 2, 0xFFFFFFFF, 0, N - 1]]).astype(np.uint32)
        qd = np.concatenate([rng.integers(0, 2000, 150), np.arange(30) * 5 + 1, [0, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0]]).astype(np.uint32)
        perm = rng.permutation(len(qs))
        qs, qd = np.ascontiguousarray(qs[perm]), np.ascontiguousarray(qd[perm])
        verts = np.concatenate([rng.integers(0, N, 60), [250, 250, 250], rng.integers(0, N, 60), [N, N + 1, 0xFFFFFFFF, N - 1, 250]]).astype(np.uint32)
        verts = np.ascontiguousarray(verts)
        wl, wg = pp_model(pp, qs, qd, verts)
        pl, pg = pp_per_partition(pp, qs, qd, verts)
        np.testing.assert_array_equal(pl, wl, err_msg=label)
        for a, b in zip(pg, wg):
            np.testing.assert_array_equal(a, b, err_msg=label)
        assert np.mean(wl != NO_EDGE) > 0.05 and len(live) > 1000
        T = len(wg[1])
        hub_len = int(np.diff(wg[0])[list(verts).index(250)])
        assert hub_len >= 400
        for qb, gs in [(1, 1), (1, 17), (13, 1), (13, 17), (1 << 20, 1 << 22)]:
            lab = f"{label}, query_block {qb}, gather_stage {gs}"
            pp.set_option("query_block", qb)
            pp.set_option("gather_stage", gs)
            np.testing.assert_array_equal(pp.lookup_edges(qs, qd), wl, err_msg=lab)
            r, d, v = pp.gather_neighbourhoods(verts)
            np.testing.assert_array_equal(r, wg[0], err_msg=lab)
            np.testing.assert_array_equal(d, wg[1], err_msg=lab)
            np.testing.assert_array_equal(v, wg[2], err_msg=lab)
            if qb == 13 and gs == 17:
                i = list(verts).index(250)

                def call(r, d, v, cap, tot):
                    return lib.pppcsr_gather_neighbourhoods(pp.h, verts.ctypes.data, len(verts), r.ctypes.data, d.ctypes.data, v.ctypes.data,
                                                            cap, ctypes.byref(tot))
                bedge = [int(wg[0][j]) for j in range(13, len(verts), 13)]
                for cap in sorted({0, 1, T - 1, T, int(wg[0][i]) + 3, int(wg[0][i]) + hub_len // 2} | {b + x for b in bedge[:4] for x in (-1, 0, 1)}):
                    check_partial_gather(call, *wg, cap)
    pp.set_option("query_block", 1 << 20)
    pp.set_option("gather_stage", 1 << 22)


# ---- nothing is written --------------------------------------------------------------------------------------------------
def test_sim_queries_write_nothing(lib, streams):
    """snapshot, a batch, every query form at small knobs, restore: the snapshot's state; the queries alone change no stat,
    no slot, no node record and no geometry"""
    n, ops = hub_graph(streams)
    e = make(lib, n)
    e.apply(ops[::3])
    e.snapshot()
    s0 = (e.state(), e.geometry())
    e.apply(np.concatenate([streams.random_stream(n, 1500, seed=45, p_delete=0.3), ops[1::3][:1500]]))
    st, geom = e.stats(), e.geometry()
    items, nodes = e.state()
    rng = np.random.default_rng(46)
    qs, qd = lookup_queries(rng, items, nodes, HUB)
    verts = gather_queries(rng, nodes, HUB)
    knobs(e, query_lookup_stage=7, query_gather_rows=3, query_gather_chunks=5, query_gather_stage=11)
    e.lookup_edges(qs, qd)
    out = np.empty(len(qs), np.uint32)
    assert e.L.ppcsr_lookup_edges_device(e.h, qs.ctypes.data, qd.ctypes.data, len(qs), out.ctypes.data) == 0
    want = model_gather(items, nodes, verts)
    for form in (gather_host, gather_device):
        check_full(full(form, e, verts, want), want, form.__name__)
        assert form(e, verts, cap=len(want[1]) // 2)[0] == ERANGE
    e.edge_exists(HUB, 4)
    e.get_neighbourhood(HUB)
    assert e.stats() == st and e.geometry() == geom
    i1, n1 = e.state()
    np.testing.assert_array_equal(i1, items)
    np.testing.assert_array_equal(n1, nodes)
    e.restore()
    (i2, n2), g2 = e.state(), e.geometry()
    assert g2 == s0[1]
    np.testing.assert_array_equal(i2, s0[0][0])
    np.testing.assert_array_equal(n2, s0[0][1])
    assert e.check_invariants() == 0


# ---- allocation failures in the read path ---------------------------------------------------------------------------------
def test_sim_query_allocation_failures(lib, streams):
    """for every device allocation a larger call makes (its staging, row, chunk and scan-scratch buffers), on a handle that
    answered a small call before: the larger call with that allocation failing reports ENOMEM or answers correctly; then the
    small call and the larger one both answer correctly (a buffer left null by a failed regrow must not be reused)"""
    pkg = load_pkg()
    n, ops = hub_graph(streams)
    adds = ops[ops[:, 2] != 0]
    rng = np.random.default_rng(47)
    counter = ctypes.c_int.in_dll(lib, "g_sim_fail_alloc")

    def fresh():
        e = pkg.PCSR(n, lib=lib)
        e.bulk_build(adds)
        return e

    e = fresh()
    items, nodes = e.state()
    sq, sd = lookup_queries(rng, items, nodes, HUB, m=90)
    lq, ld = lookup_queries(rng, items, nodes, HUB, m=3000)
    sv = np.ascontiguousarray(rng.integers(0, n, 40).astype(np.uint32))
    lv = np.ascontiguousarray(np.concatenate([rng.integers(0, n, 4500), np.full(70, HUB)]).astype(np.uint32)[rng.permutation(4570)])
    assert gather_chunks(nodes, lv).sum() > 2 * 4096 and len(lv) > 4096  # (the scans of the large gather need scratch)
    want = {"s": (model_lookup(items, n, sq, sd), model_gather(items, nodes, sv)),
            "l": (model_lookup(items, n, lq, ld), model_gather(items, nodes, lv))}

    def small():
        np.testing.assert_array_equal(e.lookup_edges(sq, sd), want["s"][0])
        check_full(gather_host(e, sv), want["s"][1], "small")

    def large(may_fail):
        rcs = []
        out = np.empty(len(lq), np.uint32)
        rc = lib.ppcsr_lookup_edges(e.h, lq.ctypes.data, ld.ctypes.data, len(lq), out.ctypes.data)
        assert rc in ((0, 2) if may_fail else (0,))
        if rc == 0:
            np.testing.assert_array_equal(out, want["l"][0])
        rcs.append(rc)
        T = len(want["l"][1][1])
        r, d, v = np.zeros(len(lv) + 1, np.uint64), np.full(T, -7, np.int32), np.zeros(T, np.uint32)
        tot = ctypes.c_uint64(0)
        rc = lib.ppcsr_gather_neighbourhoods(e.h, lv.ctypes.data, len(lv), r.ctypes.data, d.ctypes.data, v.ctypes.data, T, ctypes.byref(tot))
        assert rc in ((0, 2) if may_fail else (0,))
        if rc == 0:
            check_full((rc, tot.value, r, np.concatenate([d, np.full(4, -7, np.int32)]), np.concatenate([v, np.full(4, 0xA5A5A5A5, np.uint32)])),
                       want["l"][1], "large")
        rcs.append(rc)
        return rcs

    # how many device allocations the larger call makes after the small one
    small()
    counter.value = 1 << 30
    large(False)
    allocs = (1 << 30) - counter.value
    lib.ppcsr_sim_fail_alloc_after(0)
    assert allocs >= 14, allocs  # 3 lookup staging, 6 row arrays, 2 output windows, 3 chunk arrays, scan scratch
    failed = 0
    for k in range(1, allocs + 1):
        e = fresh()
        small()
        lib.ppcsr_sim_fail_alloc_after(k)
        try:
            rcs = large(True)
        finally:
            lib.ppcsr_sim_fail_alloc_after(0)
        failed += 2 in rcs
        small()
        large(False)
        i1, n1 = e.state()
        np.testing.assert_array_equal(i1, items)
        np.testing.assert_array_equal(n1, nodes)
    assert failed == allocs  # (every one of those allocations was hit)
