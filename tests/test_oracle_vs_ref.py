"""CPU: the oracle restatement against the UNMODIFIED reference.  What the reference computes on these streams (geometry,
a digest of the whole state, of sampled neighbourhoods and of its BFS / PageRank templates' results) is stored in
tests/golden/ref_digests.json, written from oracle/_ref (the reference compiled where it lies) by
tests/golden/make_ref_digests.py, which runs the same case definitions through the reference."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, digest, reference_consumers
from oracle_lib import Oracle

REF_DIGESTS = os.path.join(GOLDEN, "ref_digests.json")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(np.int64(a.size).tobytes())
        h.update(a.tobytes())
    return h.hexdigest()


def fingerprint(eng, n):
    """geometry, sha256 of edges[] + nodes[] (tests/helpers.digest) and of every (n / 50)-th vertex's neighbourhood"""
    geom = [int(x) for x in eng.geometry()]
    items, nodes = eng.state()
    nbs = [eng.get_neighbourhood(v) for v in range(0, n, max(1, n // 50))]
    return {"geometry": geom, "state": digest(items, nodes, geom), "neighbourhoods": _sha(*nbs)}


def _run(make, n, ops, lock=True):
    e = make(n, lock)
    e.apply(ops)
    fp = fingerprint(e, n)
    e.close()
    return fp


def random_mixed(make, streams, seed, lock):
    n = [30, 200, 1000, 3000, 5000, 20000][seed]
    core = streams.random_stream(n, 40000, seed=100 + seed)
    fresh = streams.random_stream(n, 15000, seed=200 + seed)
    ops = np.concatenate([core, streams.mixed_existing_stream(core, fresh, seed=300 + seed)])
    return [_run(make, n, ops, lock)]


def delete_everything_then_reinsert(make, streams):
    n = 300
    a = streams.random_stream(n, 30000, seed=5)
    d = a.copy()
    d[:, 2] = 0
    return [_run(make, n, np.concatenate([a, d, a[::-1]]))]


def hub_and_last_vertex(make, streams):
    m = 20000
    hub = np.stack([np.full(m, 9), streams.uniform_ints(3, m, 1 << 30), np.ones(m)], 1).astype(np.uint32)  # last vertex
    out = [_run(make, 10, hub)]
    hub[:, 0] = 0  # first vertex
    out.append(_run(make, 10, hub))
    hub[:, 0] = streams.uniform_ints(4, m, 3) + 7  # tail hubs
    out.append(_run(make, 10, hub))
    return out


def rmat_skew(make, streams):
    s, d = streams.rmat_edges(13, 150000, seed=1)
    core = streams.adds(s, d)
    s2, d2 = streams.rmat_edges(13, 40000, seed=2)
    ops = np.concatenate([core, streams.mixed_existing_stream(core, streams.adds(s2, d2), seed=3)])
    return [_run(make, 1 << 13, ops)]


def edge_values_and_add_node(make, streams):
    e = make(0, True)
    for _ in range(20):
        e.add_node()
    ops = streams.random_stream(20, 5000, seed=9, p_delete=0.3)
    ops[:, 2] *= streams.uniform_ints(10, 5000, 1000) + 1
    e.apply(ops)
    for _ in range(7):
        e.add_node()
    e.apply(streams.random_stream(27, 5000, seed=10, p_delete=0.1))
    fp = fingerprint(e, 27)
    e.close()
    return [fp]


def consumer_graph(make, streams):
    """RMAT scale 14, 200 K edges, every sixth deleted again; returns (engine, starts, node values)"""
    scale, m = 14, 200_000
    n = 1 << scale
    s, d = streams.rmat_edges(scale, m, seed=51)
    ops = streams.adds(s, d)
    dele = ops[::6].copy()
    dele[:, 2] = 0
    e = make(n, True)
    e.apply(np.concatenate([ops, dele]))
    vals = (streams.uniform_ints(52, n, 1000).astype(np.float32) / np.float32(3.0)).astype(np.float32)
    return e, (0, 5, int(s[4321])), vals


def cases(streams):
    """key -> function(make) -> list of fingerprints; make(n, lock_search) builds an engine (Oracle or the reference)"""
    out = {f"random_mixed[{seed}-{lock}]": (lambda make, seed=seed, lock=lock: random_mixed(make, streams, seed, lock))
           for lock in (True, False) for seed in range(6)}
    for f in (delete_everything_then_reinsert, hub_and_last_vertex, rmat_skew, edge_values_and_add_node):
        out[f.__name__] = lambda make, f=f: f(make, streams)
    return out


@pytest.fixture(scope="module")
def ref():
    return json.load(open(REF_DIGESTS))


def _check(ref, streams, key):
    got = cases(streams)[key](lambda n, lock: Oracle(n, lock_search=lock))
    assert len(got) == len(ref[key]), key
    for i, (g, r) in enumerate(zip(got, ref[key])):
        assert g["geometry"] == r["geometry"], f"{key} #{i}: geometry {g['geometry']} vs the reference's {r['geometry']}"
        assert g["state"] == r["state"], f"{key} #{i}: edges[] / nodes[] differ from the reference's"
        assert g["neighbourhoods"] == r["neighbourhoods"], f"{key} #{i}: neighbourhoods differ from the reference's"


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("lock", [True, False])
def test_random_mixed(ref, streams, seed, lock):
    _check(ref, streams, f"random_mixed[{seed}-{lock}]")


def test_delete_everything_then_reinsert(ref, streams):
    _check(ref, streams, "delete_everything_then_reinsert")


def test_hub_and_last_vertex(ref, streams):
    _check(ref, streams, "hub_and_last_vertex")


def test_rmat_skew(ref, streams):
    _check(ref, streams, "rmat_skew")


def test_edge_values_and_add_node(ref, streams):
    _check(ref, streams, "edge_values_and_add_node")


def test_consumer_restatement_vs_reference_templates_rmat(ref, streams):
    """the reference's bfs.h / pagerank.h templates on the reference PCSR vs tests/helpers.py:reference_consumers on the
    oracle, on a larger graph than the committed fixture (RMAT scale 14, 200 K edges, deletes): BFS levels equal, PageRank
    bit for bit"""
    o, starts, vals = consumer_graph(lambda n, lock: Oracle(n, lock_search=lock), streams)
    want = ref["consumers_rmat14"]
    for start in starts:
        lv, pr = reference_consumers(o, start, vals)
        assert _sha(lv) == want[f"bfs_{start}"], f"BFS levels from {start} differ from the reference template's"
    assert _sha(pr) == want["pagerank"], "PageRank differs from the reference template's"
    o.close()
