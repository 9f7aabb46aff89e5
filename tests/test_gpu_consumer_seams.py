"""GPU: every device consumer over one small graph that sits on the seams of what the consumers share — the streaming load of
the concatenated chunk space, the owner searches, the hub hand-off and the frontier threshold of the hybrid loop — on one
array, on three, and on a table that holds an EMPTY partition (which only the emulator suites met so far).  Everything is
compared with the host models of tests/ (consumers_model, paths_model, kcore_model, triangles_model), built from the exported
partition states."""
import numpy as np
import pytest

from consumers_model import global_edges, model_bfs, model_pagerank, num_neighbors, partition_states
from helpers import load_pkg
from kcore_model import model_kcore
from paths_model import global_edges_valued, model_components, model_sssp
from triangles_model import model_common_neighbours, model_triangles

pytestmark = pytest.mark.gpu

N, HUB = 6000, 7
WAVE_SLOTS = 4096  # longest slot range (and adjacency list) one wave walks on its own


def seam_graph(streams):
    """the graph of test_sim_kcore_hub_and_long_list: a hub with 5000 leaves that is also adjacent to 60 members of a clique
    K_100, stored in the upper orientation (the hub's small id makes it the source of nearly all its pairs), with edge values
    in [1, 1000]"""
    rng = np.random.default_rng(1)
    others = rng.permutation(np.setdiff1d(np.arange(N), [HUB]))
    leaves, kq = others[:5000], others[5000:5100]
    i, j = np.triu_indices(len(kq), 1)
    pairs = np.concatenate([np.stack([np.full(5000, HUB), leaves], axis=1), np.stack([kq[i], kq[j]], axis=1),
                            np.stack([np.full(60, HUB), kq[:60]], axis=1)])
    ops = np.stack([pairs.min(axis=1), pairs.max(axis=1), np.ones(len(pairs), np.int64)], axis=1).astype(np.uint32)
    ops = ops[rng.permutation(len(ops))]
    ops[:, 2] = streams.uniform_ints(77, len(ops), 1000) + np.uint32(1)
    return ops, leaves, kq


def check_form(pp, label, leaves, kq):
    """all seven consumers against the models; the conditions on the input from the models; nothing written"""
    n = pp.get_n()
    assert n == N
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst, val = global_edges_valued(states)
    s2, d2 = global_edges(states)
    assert np.array_equal(src, s2) and np.array_equal(dst, d2)
    beginning, end, _ = pp.getNode(HUB)
    assert end - beginning > WAVE_SLOTS, (label, beginning, end)  # the per-vertex kernels hand the hub to the streaming pass
    leaf = int(leaves.min())
    assert leaf < HUB  # (its one stored pair is (leaf, hub): the walk from it meets the hub on its second level)
    widest = 0
    for start in (HUB, leaf):
        want, w = model_bfs(src, dst, n, start)
        widest = max(widest, w)
        np.testing.assert_array_equal(pp.bfs(start), want, err_msg=f"{label}: bfs from {start}")
        np.testing.assert_array_equal(pp.sssp(start), model_sssp(src, dst, val, n, start), err_msg=f"{label}: sssp from {start}")
    assert widest >= max(64, n // 256) == 64, (label, widest)  # both sides of the frontier threshold: 1, then 5060, then small
    np.testing.assert_array_equal(pp.components(), model_components(src, dst, n), err_msg=f"{label}: components")
    core, kmax = pp.kcore()
    want = model_kcore(src, dst, n)
    np.testing.assert_array_equal(core, want, err_msg=f"{label}: core")
    assert kmax == want.max() == 99 and want[HUB] == 60, label  # (the hub's list of 5060 entries: k_kc_peel_long)
    tri_want, total_want = model_triangles(src, dst, n)
    tri, total = pp.triangles()
    np.testing.assert_array_equal(tri, tri_want, err_msg=f"{label}: tri")
    assert total == total_want and total >= 100 * 99 * 98 // 6, (label, total, total_want)
    none, total = pp.triangles(per_vertex=False)
    assert none is None and total == total_want, label
    # 256 pairs: random ones with vertices >= n among them, the hub with clique members, with itself and with a vertex >= n,
    # and the vertex at which the empty partition of the last form starts and ends
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, n + 40, 256).astype(np.uint32), rng.integers(0, n + 40, 256).astype(np.uint32)
    a[:8] = [HUB, HUB, kq[0], kq[61], HUB, n + 3, 100, 100]
    b[:8] = [kq[0], kq[70], kq[1], HUB, HUB, HUB, 100, HUB]
    assert (a >= n).sum() >= 2 and (b >= n).sum() >= 1
    cn_want = model_common_neighbours(src, dst, n, a, b)
    assert cn_want[4] > WAVE_SLOTS and cn_want[:4].any() and not cn_want[5], cn_want[:8]  # (the hub with itself: a range beyond one wave's)
    np.testing.assert_array_equal(pp.common_neighbours(a, b), cn_want, err_msg=f"{label}: common neighbours")
    vals = (np.random.default_rng(4).integers(1, 64, n) / 8.0).astype(np.float32)  # (strictly positive: no 0 / 0)
    got = pp.pagerank(vals)
    ref = model_pagerank(src, dst, num_neighbors(states), vals)
    assert got.tobytes() == ref.tobytes(), f"{label}: pagerank differs at {np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0][:10]}"
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label


def run_forms(pkg, adds_ptr, count, leaves, kq):
    for P in (1, 3, 4):
        pp = pkg.PPPCSR(N, numDomain=1, partitionsPerDomain=P)
        pp.bulk_build_device(adds_ptr, count)
        label = f"P={P}"
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # partition 1 is empty: it owns no vertex and no edge
            assert pp.partition(1).get_n() == 0 and pp.get_partiton(100) == 2
            label += " with an empty partition"
        check_form(pp, label, leaves, kq)
        pp.close()


def test_consumer_seams(streams):
    import torch
    pkg = load_pkg()
    pkg.load_library()
    ops, leaves, kq = seam_graph(streams)
    t = torch.from_numpy(np.ascontiguousarray(ops).view(np.int32)).cuda()
    torch.cuda.synchronize()
    run_forms(pkg, t.data_ptr(), len(ops), leaves, kq)
