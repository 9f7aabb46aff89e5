"""GPU: pppcsr_bfs / pppcsr_pagerank (the reference's bfs.h / pagerank.h templates with T = PPPCSR) on MI355X, all
partitions on one device: against the reference's own template results (tests/golden/consumers_rmat12.npz), against the
numpy model of the templates at RMAT scale 18 (tests/consumers_model.py), against one PCSR holding the same graph at config
#2's size, and through the C++ host overloads (tests/cpp/test_pppcsr_consumers.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from consumers_model import global_edges, last_slot_free, model_bfs, model_pagerank, num_neighbors, partition_states
from helpers import ROOT, golden, load_pkg

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


def check_model(pp, starts, vals, label):
    n = pp.get_n()
    states = partition_states(pp)
    src, dst = global_edges(states)
    for s in starts:
        np.testing.assert_array_equal(pp.bfs(s), model_bfs(src, dst, n, s)[0], err_msg=f"{label}: bfs from {s}")
    got = pp.pagerank(vals)
    ref = model_pagerank(src, dst, num_neighbors(states), vals)
    assert got.tobytes() == ref.tobytes(), f"{label}: pagerank differs at {np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0][:10]}"
    after = partition_states(pp)  # nothing written
    for (_, i0, n0), (_, i1, n1) in zip(states, after):
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1), label


@pytest.mark.parametrize("P", [1, 4, 8])
def test_pppcsr_consumers_golden_from_reference_templates(pkg, P):
    """the ops of consumers_rmat12 routed over P partitions on device 0: levels and PageRank (both value vectors) of the
    reference's own templates on its single PCSR"""
    g = golden("consumers_rmat12")
    n = int(g["n"])
    one = pkg.PCSR(n)
    one.apply(g["ops"])
    assert last_slot_free(one.state()[0])  # (the slot precondition: the reference's layout ...)
    one.close()
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P, devices=[0])
    pp.apply(g["ops"])
    assert all(last_slot_free(i) for _, i, _ in partition_states(pp))  # (... and every partition's)
    for i, start in enumerate(g["starts"]):
        np.testing.assert_array_equal(pp.bfs(int(start)), g["levels"][i])
    assert pp.pagerank(g["node_values"]).tobytes() == g["pagerank"].tobytes()
    assert pp.pagerank(np.ones(n, np.float32)).tobytes() == g["pagerank_ones"].tobytes()


def test_pppcsr_consumers_model_rmat18(pkg, streams):
    """P = 8: a 2 M-edge RMAT core and a mixed stream, add_node, a repartition to balanced_starts; then a graph with a hub
    of 2^20 edges (wider than any wave walks on its own), bulk-built on a fresh PPPCSR"""
    n, P = 1 << 18, 8
    s, d = streams.rmat_edges(18, 2_000_000, seed=31)
    core = streams.adds(s, d)
    s2, d2 = streams.rmat_edges(18, 300_000, seed=32)
    mixed = streams.mixed_existing_stream(core, streams.adds(s2, d2 + np.uint32(7)), seed=33)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    pp.apply(core)
    pp.apply(mixed)
    pp.add_node()
    pp.apply(np.array([[n, 1, 1], [2, n, 1]], np.uint32))
    pp.add_node()  # (isolated)
    vals = ((np.arange(n + 2) % 13 + 1) / 4.0).astype(np.float32)
    starts = [0, int(core[0, 0]), n // 2 + 5, n - 1, n, n + 1]
    check_model(pp, starts, vals, "rmat18")
    pp.repartition(pp.balanced_starts())
    check_model(pp, starts, vals, "rmat18 repartitioned")
    pp.close()

    m, nh = 1 << 20, 1 << 21
    hub = 3 * nh // 8 + 11
    rng = np.random.default_rng(5)
    s3, d3 = streams.rmat_edges_folded(nh, 21, 2_000_000, seed=34)
    adds = np.concatenate([streams.adds(s3, d3), streams.adds(np.full(m, hub, np.uint32), rng.permutation(nh)[:m].astype(np.uint32))])
    pp = pkg.PPPCSR(nh, numDomain=1, partitionsPerDomain=P)
    t = to_device(adds)
    pp.bulk_build_device(t.data_ptr(), len(adds))
    node = pp.getNode(hub)
    assert node[1] - node[0] > m
    check_model(pp, [hub, 0, int(s3[0])], np.ones(nh, np.float32), "hub")


def test_pppcsr_consumers_match_one_engine_config2(pkg, streams):
    """config #2's graph (RMAT scale 20, 10 M core edges, bulk-built) and a 1 M mixed stream, on 8 partitions and on one
    PCSR: equal levels, bitwise-equal PageRank"""
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
    assert last_slot_free(one.state()[0])
    assert all(last_slot_free(i) for _, i, _ in partition_states(pp))
    for start in (0, int(s[1]), n - 1):
        a, ms_pp = pp.bfs(start, with_ms=True)
        b, ms_one = one.bfs(start, with_ms=True)
        np.testing.assert_array_equal(a, b)
    for vals in (np.ones(n, np.float32), ((np.arange(n) % 29 + 1) / 8.0).astype(np.float32)):
        assert pp.pagerank(vals).tobytes() == one.pagerank(vals).tobytes()


def test_cpp_pppcsr_consumer_overloads():
    """bfs(pp, s) / pagerank(pp, v) resolve to the device and equal the host templates bfs<PPPCSR> / pagerank<PPPCSR, float>"""
    lib_dir = os.path.join(ROOT, "parallel-packed-csr_amd", "csrc")
    exe = os.path.join(ROOT, "tests", "cpp", "test_pppcsr_consumers")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "parallel-packed-csr_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_pppcsr_consumers.cpp"),
                    "-L" + lib_dir, "-lppcsr_hip", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
