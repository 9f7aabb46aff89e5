"""Shared test helpers: fixture loading, state digests, package loading."""
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
PKG_DIR = os.path.join(ROOT, "parallel-packed-csr_amd")


def _load(name, path):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)]
                                                  if path.endswith("__init__.py") else None)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_streams():
    return _load("ppcsr_streams", os.path.join(PKG_DIR, "streams.py"))


def load_pkg():
    """the product package (directory name has a hyphen, so it is loaded by path as `ppcsr_amd`)."""
    return _load("ppcsr_amd", os.path.join(PKG_DIR, "__init__.py"))


def hip_runtime():
    """ctypes handle of the HIP runtime this process holds already, for hipMalloc / hipMemcpy / hipFree in GPU tests; call it after
    load_pkg().load_library().  Where PyTorch is installed the engine shares the wheel's runtime (__init__.py _share_hip_runtime:
    loaded by path, symbols global, SONAME libamdhip64.so.<major>), and asking the loader for "libamdhip64.so" by name would bring
    in a SECOND runtime, the system's — which need not even load beside the wheel's HSA runtime.  So: the global symbols first."""
    import ctypes
    g = ctypes.CDLL(None)
    return g if hasattr(g, "hipMalloc") else ctypes.CDLL("libamdhip64.so")


def digest(items, nodes, geom):
    h = hashlib.sha256()
    h.update(np.array(geom, np.int64).tobytes())
    h.update(np.ascontiguousarray(items).tobytes())
    h.update(np.ascontiguousarray(nodes).tobytes())
    return h.hexdigest()


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


GOLDEN_SINGLE = [
    "hub_1e4_insert_then_delete", "random_2e4_n1000", "insert_50k_n2000", "mixed_existing_80k_n2000",
    "rmat12_core60k_mixed40k", "random_2e4_n1000_lockfree", "dense_n40_grow_shrink", "add_node_empty_then_edges",
]


def replay_golden(make_engine, name, check_every=True):
    """Apply fixture `name` to make_engine(n, lock_search) checkpoint by checkpoint; return the engine.
    Asserts geometry + digest at every checkpoint and the raw state when stored."""
    g = golden(name)
    n, lock = int(g["n"]), bool(int(g["lock_search"]))
    eng = make_engine(n, lock)
    if name == "add_node_empty_then_edges":
        for _ in range(5):
            eng.add_node()
    ops, cps = g["ops"], g["checkpoints"]
    prev = 0
    for i, c in enumerate(cps):
        eng.apply(ops[prev:c])
        prev = int(c)
        if check_every or i == len(cps) - 1:
            geom = eng.geometry()
            assert tuple(geom) == tuple(int(x) for x in g["geoms"][i]), f"{name}: geometry at op {c}: {geom} vs {g['geoms'][i]}"
            items, nodes = eng.state()
            assert digest(items, nodes, geom) == str(g["digests"][i]), f"{name}: state digest differs at checkpoint {i} (op {c})"
    if "items" in g.files:
        items, nodes = eng.state()
        np.testing.assert_array_equal(items, g["items"])
        np.testing.assert_array_equal(nodes, g["nodes"])
    return eng


def reference_consumers(oracle, start, node_values):
    """src/utility/bfs.h:15-36 and src/utility/pagerank.h:15-29 evaluated on an oracle's state with numpy: BFS levels
    (uint32, 0xFFFFFFFF = unreachable) and the one-step PageRank push with fp32 additions in the reference's order
    (np.add.at applies its updates one by one in index order = ascending source, neighbours in slot order)."""
    import numpy as np
    items, nodes = oracle.state()
    n = len(nodes)
    live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF)
    live[-1] = False  # slot N-1 is never part of a neighbourhood
    src = items[live, 0].astype(np.int64)
    dst = items[live, 1].astype(np.int64)
    # BFS by levels
    lv = np.full(n, 0xFFFFFFFF, np.uint32)
    lv[start] = 0
    order = np.argsort(src, kind="stable")
    s_sorted, d_sorted = src[order], dst[order]
    rows = np.searchsorted(s_sorted, np.arange(n + 1))
    front = np.array([start], np.int64)
    level = 0
    while len(front):
        nb = np.concatenate([d_sorted[rows[u]:rows[u + 1]] for u in front]) if len(front) else np.empty(0, np.int64)
        nb = nb[nb < n]
        nb = np.unique(nb[lv[nb] == 0xFFFFFFFF])
        level += 1
        lv[nb] = level
        front = nb
    # PageRank push: edges are visited in array order == (source ascending, slot order)
    vals = np.asarray(node_values, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        contrib = (vals / nodes[:, 2].astype(np.float32)).astype(np.float32)
    out = np.zeros(n, np.float32)
    ok = dst < n
    np.add.at(out, dst[ok], contrib[src[ok]])
    return lv, out


import numpy as np  # noqa: E402


def edge_view(items, nodes):
    """layout-independent view of a PCSR state: CSR (row lengths, dests, values) + num_neighbors"""
    live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF)
    live[-1] = False
    deg = np.bincount(items[live, 0], minlength=len(nodes))
    return deg, items[live, 1], items[live, 2], nodes[:, 2]


def check_pma_invariants(items, nodes):
    N, n = len(items), len(nodes)
    live = items[:, 2] != 0
    nul = items[~live]
    assert (nul[:, 0] == 0xFFFFFFFF).all() and (nul[:, 1] == 0).all()
    sent = live & (items[:, 1] == 0xFFFFFFFF)
    pos = np.nonzero(sent)[0]
    assert len(pos) == n
    np.testing.assert_array_equal(items[pos, 0], np.arange(n, dtype=np.uint32))
    np.testing.assert_array_equal(nodes[:, 0], pos.astype(np.uint32))
    np.testing.assert_array_equal(nodes[:-1, 1], nodes[1:, 0])
    assert nodes[-1, 1] == N - 1
    e = np.nonzero(live & ~sent)[0]
    owner = np.searchsorted(pos, e, side="right") - 1
    np.testing.assert_array_equal(items[e, 0], owner.astype(np.uint32))
    key = items[e, 0].astype(np.uint64) << np.uint64(32) | items[e, 1].astype(np.uint64)
    assert (np.diff(key.astype(np.int64)) > 0).all()  # sorted and unique inside every neighbourhood


# sources of 80 ascending-dest inserts into the last three of 4096 vertices: the 47th makes slide_right run off the end
# of the array (PCSR.cpp:347-351) — found by tools/fuzz_parity.py (seed 5069); the reference recovers through slide_left
SLIDE_OFF_END_SRC = [4094, 4094, 4094, 4093, 4094, 4095, 4094, 4095, 4094, 4093, 4093, 4094, 4095, 4095, 4094, 4095, 4093, 4095, 4094, 4094, 4094, 4093, 4093, 4095, 4094, 4093, 4094, 4093, 4095, 4095, 4093, 4094, 4094, 4095, 4094, 4093, 4095, 4095, 4093, 4093, 4094, 4093, 4095, 4094, 4095, 4093, 4094, 4093, 4095, 4093, 4095, 4095, 4095, 4093, 4093, 4095, 4093, 4093, 4095, 4095, 4093, 4094, 4094, 4094, 4094, 4093, 4095, 4094, 4094, 4093, 4095, 4094, 4094, 4095, 4094, 4094, 4095, 4094, 4094, 4093]


def slide_off_end_stream():
    import numpy as np
    src = np.array(SLIDE_OFF_END_SRC, np.uint32)
    return np.stack([src, np.arange(len(src), dtype=np.uint32), np.ones(len(src), np.uint32)], 1)


def live_triples(items, base=0):
    """every edge of a raw edges[] export as (src + base, dest, value), array order (sentinels and empty slots dropped; the
    last slot included — see Engine::export_triples_device)"""
    it = np.asarray(items, np.uint32).reshape(-1, 3)
    live = (it[:, 2] != 0) & (it[:, 1] != 0xFFFFFFFF) & (it[:, 2] != 0xFFFFFFFF)
    out = it[live].copy()
    out[:, 0] += np.uint32(base)
    return out


def check_repartitioned(new_states, old_states, old_starts, new_starts, total_n, build_bulk=None, lock_search=True):
    """the rule of pppcsr_repartition (include/ppcsr.h) checked on raw states: new_states[k] / old_states[k] = (items, nodes) of
    partition k after / before.  A partition whose vertex range did not change is untouched bit for bit.  A changed one equals
    the exact host model of the bulk build (tests/bulk_model.py) of the edges that fall into its new range — partition-local src,
    ascending (src, dest), into the array a fresh Oracle of that many vertices has — or, when no edge falls into it, that fresh
    Oracle's state: nothing is routed to it, so nothing builds it.  Except for num_neighbors, which every vertex carries over
    unchanged (it is a counter of calls, not the degree).  build_bulk(size, adds) -> (items, nodes), when given, replaces the
    model as the expectation.  Returns the expected (items, nodes) of every partition (None for one without vertices)."""
    from bulk_model import bulk_model
    from oracle_lib import Oracle
    P = len(old_states)
    end = lambda st, k: int(st[k + 1]) if k + 1 < P else int(total_n)
    changed = [int(old_starts[k]) != int(new_starts[k]) or end(old_starts, k) != end(new_starts, k) for k in range(P)]
    moved = [live_triples(old_states[k][0], int(old_starts[k])) for k in range(P) if changed[k]]
    moved = np.concatenate(moved) if moved else np.zeros((0, 3), np.uint32)
    nn_old = np.concatenate([np.asarray(old_states[k][1], np.uint32).reshape(-1, 3)[:, 2] for k in range(P)])  # by global vertex
    want = []
    for k in range(P):
        it, nd = new_states[k]
        nd = np.asarray(nd, np.uint32).reshape(-1, 3)
        lo, hi = int(new_starts[k]), end(new_starts, k)
        assert len(nd) == hi - lo, f"partition {k}: {len(nd)} vertices, range [{lo}, {hi})"
        if not changed[k]:
            assert np.array_equal(it, old_states[k][0]) and np.array_equal(nd, np.asarray(old_states[k][1], np.uint32).reshape(-1, 3)), f"partition {k} was to stay untouched"
            want.append((old_states[k][0], old_states[k][1]) if hi > lo else None)
            continue
        sub = moved[(moved[:, 0] >= lo) & (moved[:, 0] < hi)].copy()
        sub[:, 0] -= np.uint32(lo)
        if hi > lo:
            if build_bulk is not None:
                eit, end_ = build_bulk(hi - lo, sub)
            else:
                fresh = Oracle(hi - lo, lock_search=lock_search)
                eit, end_ = bulk_model(hi - lo, fresh.geometry()[0], sub, lock_search=lock_search) if len(sub) else fresh.state()
            end_ = np.asarray(end_, np.uint32).reshape(-1, 3).copy()
            end_[:, 2] = nn_old[lo:hi]
            want.append((eit, end_))
            assert np.array_equal(it, eit), f"partition {k}: edges[] differ from the bulk build of its new range"
            assert np.array_equal(nd[:, :2], end_[:, :2]), f"partition {k}: vertex ranges differ from the bulk build"
        np.testing.assert_array_equal(nd[:, 2], nn_old[lo:hi], err_msg=f"partition {k}: num_neighbors not carried over")
        if hi > lo:
            check_pma_invariants(np.asarray(it, np.uint32).reshape(-1, 3), nd)
        else:
            want.append(None)
        if len(sub):
            np.testing.assert_array_equal(live_triples(it, lo), sub + np.array([lo, 0, 0], np.uint32))
    return want


# ---- exact models of the batched reads (ppcsr_lookup_edges / ppcsr_gather_neighbourhoods) on an exported state ------------
NO_EDGE = 0xFFFFFFFF
ERANGE = 6  # PPCSR_STATUS_ERANGE


def _live(items):
    return (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)


def model_lookup(items, n, qs, qd):
    """value of edge (qs[i], qd[i]) or NO_EDGE, from the sorted src << 32 | dst keys of the live slots (uint64)"""
    live = _live(items)
    keys = (items[live, 0].astype(np.uint64) << np.uint64(32)) | items[live, 1].astype(np.uint64)
    vals = items[live, 2]
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    assert np.all(np.diff(keys) > 0), "an edge in two live slots"
    qk = (qs.astype(np.uint64) << np.uint64(32)) | qd.astype(np.uint64)
    pos = np.minimum(np.searchsorted(keys, qk), max(len(keys) - 1, 0))
    hit = (len(keys) > 0) & (keys[pos] == qk) & (qs < n) if len(keys) else np.zeros(len(qk), bool)
    return np.where(hit, vals[pos] if len(keys) else 0, np.uint32(NO_EDGE)).astype(np.uint32)


def model_gather(items, nodes, verts):
    """(row_offsets uint64[k + 1], dests int32, values uint32): the live slots of (beginning, end) of every queried vertex"""
    n = len(nodes)
    v = verts.astype(np.int64)
    ok = v < n
    lo = np.zeros(len(v), np.int64)
    hi = np.zeros(len(v), np.int64)
    lo[ok] = nodes[v[ok], 0].astype(np.int64) + 1
    hi[ok] = nodes[v[ok], 1].astype(np.int64)
    lens = np.maximum(hi - lo, 0)
    tot = int(lens.sum())
    idx = np.repeat(lo - np.cumsum(lens) + lens, lens) + np.arange(tot, dtype=np.int64)
    rid = np.repeat(np.arange(len(v)), lens)
    keep = items[idx, 2] != 0
    sel = idx[keep]
    cnt = np.bincount(rid[keep], minlength=len(v))
    rows = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    return rows, items[sel, 1].astype(np.int32), items[sel, 2]


def gather_chunks(nodes, verts):
    """64-slot chunks of every queried vertex's range (what k_gather_rows counts), int64"""
    n = len(nodes)
    v = verts.astype(np.int64)
    ok = v < n
    lens = np.zeros(len(v), np.int64)
    lens[ok] = np.maximum(nodes[v[ok], 1].astype(np.int64) - nodes[v[ok], 0].astype(np.int64) - 1, 0)
    return (lens + 63) // 64


def gather_blocks(nodes, verts, rows=1 << 20, chunks=1 << 22):
    """the first row of every block a gather splits the queries into (Engine::gather_neighbourhoods / gather_prepare with
    query_gather_rows = rows, query_gather_chunks = chunks), then k: a block takes up to `rows` rows, cut back to the longest
    prefix whose chunks fit `chunks` (at least one row)"""
    nch = gather_chunks(nodes, verts)
    k = len(verts)
    cs = np.concatenate([[0], np.cumsum(nch)])
    out, i0 = [0], 0
    while i0 < k:
        kb = min(k - i0, rows)
        if cs[i0 + kb] - cs[i0] > chunks and kb > 1:
            kb = max(int(np.searchsorted(cs[i0:i0 + kb + 1] - cs[i0], chunks, side="right")) - 1, 1)
        i0 += kb
        out.append(i0)
    return np.array(out, np.int64)


def check_partial_gather(call, full_rows, full_dests, full_vals, cap, canary=-7):
    """call(rows, dests, vals, cap, total) issues the gather into the given numpy arrays (total: a ctypes.c_uint64) and returns
    the status: the first cap edges are the full result's, nothing past them is written, the total and the row offsets are
    complete, and the status is ERANGE exactly when cap < total"""
    import ctypes
    T = len(full_dests)
    rows = np.zeros(len(full_rows), np.uint64)
    dests = np.full(T + 8, canary, np.int32)
    vals = np.full(T + 8, 0xA5A5A5A5, np.uint32)
    tot = ctypes.c_uint64(0)
    rc = call(rows, dests, vals, cap, tot)
    assert rc == (ERANGE if cap < T else 0), (rc, cap, T)
    assert tot.value == T, (tot.value, T)
    np.testing.assert_array_equal(rows, full_rows, err_msg=f"row offsets, cap {cap}")
    m = min(cap, T)
    np.testing.assert_array_equal(dests[:m], full_dests[:m], err_msg=f"dests, cap {cap}")
    np.testing.assert_array_equal(vals[:m], full_vals[:m], err_msg=f"values, cap {cap}")
    assert np.all(dests[m:] == canary) and np.all(vals[m:] == 0xA5A5A5A5), f"written past cap {cap}"
