"""Small constructed graphs that reach the glue code around the intersection routines — tri_item, tri_credit, the deferred list,
the quarter-chunk masks of k_tri_long, k_common_neighbours' choice of routine — shared by the emulator module and the GPU module.
What the graph must contain is asserted from the exported states by triangles_model.routes; results are compared exactly with
model_triangles / model_common_neighbours."""
import numpy as np

from consumers_model import global_edges, partition_states
from triangles_model import LANE_SLOTS, WAVE_SLOTS, assert_routes, model_common_neighbours, model_triangles, routes, wave_route

N = 4000
HUBS = 16
# a hub's edges to vertices of the graph, and beyond n: every other hub as the first pair, the others as the second
HUB_INSIDE, HUB_OUTSIDE, HUB_INSIDE_FEW, HUB_OUTSIDE_MANY = 1800, 1500, 300, 3400


def graph_adds(streams, n=N, seed=7):
    """adds of: 16 hubs (ids spread over the lower half) pointing upward — to every later hub, to vertices above them and to ids
    beyond n (stored, never counted: they lengthen the range behind the counted edges).  Every other hub has 1800 edges inside
    and 1500 beyond, so that `aend - s` passes 4096 AT a counted edge while the range stays longer than 4096 + 64, at any fill
    between 3/8 and 3/4 a bulk build leaves; the others have 300 inside and 3400 beyond: every counted edge of theirs is deferred; a sweep of degrees 1 .. 80 twice over; a few vertices of some hundred edges; a band of overlapping small triangles; a dense folded-RMAT core; a self-loop"""
    rng = np.random.default_rng(seed)
    hubs = [3 + i * (n // 2 // HUBS) for i in range(HUBS)]
    parts = []
    for i, h in enumerate(hubs):
        above = np.arange(h + 1, n)
        n_in, n_out = (HUB_INSIDE, HUB_OUTSIDE) if i % 2 == 0 else (HUB_INSIDE_FEW, HUB_OUTSIDE_MANY)
        inside = np.union1d(rng.choice(above, n_in, replace=False), np.array(hubs[i + 1:], np.int64))
        outside = n + rng.choice(4 * n_out, n_out, replace=False)
        d = np.concatenate([inside, outside])
        parts.append(streams.adds(np.full(len(d), h, np.uint32), d.astype(np.uint32)))
    for start in (40, 7 * n // 10):
        for v in range(start, start + 160):
            if v in hubs:
                continue
            deg = (v - start) // 2 + 1
            d = rng.choice(np.arange(v + 1, n), deg, replace=False)
            parts.append(streams.adds(np.full(deg, v, np.uint32), d.astype(np.uint32)))
    for j, v in enumerate(range(n // 3, n // 3 + 10)):
        deg = 150 + 120 * j
        d = rng.choice(np.arange(v + 1, n), deg, replace=False)
        parts.append(streams.adds(np.full(deg, v, np.uint32), d.astype(np.uint32)))
    band = np.arange(n - 300, n - 200, dtype=np.uint32)  # triangles (v, v + 1, v + 2) of neighbouring two-edge vertices: many
    parts += [streams.adds(band, band + np.uint32(1)), streams.adds(band, band + np.uint32(2))]  # credited sources in one chunk
    s, d = streams.rmat_edges_folded(n, 12, 40000, seed=seed + 1)
    parts.append(streams.adds(s, d))
    parts.append(np.array([[5, 5, 1]], np.uint32))
    ops = np.concatenate(parts)
    _, first = np.unique(ops[:, 0].astype(np.int64) * (1 << 32) + ops[:, 1], return_index=True)
    return np.ascontiguousarray(ops[np.sort(first)]), hubs


def build(pkg, lib, streams, P, emulator=False):
    """the graph on P partitions, bulk-built (lib: the library to load the engine from; None: the in-tree HIP build)"""
    pp = pkg.PPPCSR(N, numDomain=1, partitionsPerDomain=P, lib=lib) if lib is not None else pkg.PPPCSR(N, numDomain=1, partitionsPerDomain=P)
    adds, hubs = graph_adds(streams)
    if emulator:
        from test_sim_pppcsr_consumers import tune
        tune(pp)
        pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
    else:
        import torch
        t = torch.from_numpy(adds.view(np.int32)).cuda()
        torch.cuda.synchronize()
        pp.bulk_build_device(t.data_ptr(), len(adds))
    # a bulk build spreads every window evenly, which leaves `aend - s` in a few residues; a stream of single updates — deletes of
    # stored edges, adds, deletes that miss — moves the slots about
    rng = np.random.default_rng(P)
    gone = adds[rng.choice(len(adds), len(adds) // 25, replace=False)].copy()
    gone[:, 2] = 0
    stream = np.concatenate([gone, streams.random_stream(N, 6000, seed=11, p_delete=0.2)])
    pp.apply(np.ascontiguousarray(stream[rng.permutation(len(stream))]))
    pp.isect_hubs = hubs
    return pp


def range_slots(states, n):
    """slots of every vertex's range as k_common_neighbours takes it: max(end, beginning + 1) - (beginning + 1)"""
    out = np.zeros(n, np.int64)
    for first, _, nodes in states:
        beg, end = nodes[:, 0].astype(np.int64) + 1, nodes[:, 1].astype(np.int64)
        out[first:first + len(nodes)] = np.maximum(end, beg) - beg
    return out


def pairs_by_route(states, n, hubs, rng):
    """common-neighbour pairs per route of k_common_neighbours: both ranges short (one lane), one just over 32 slots (the wave,
    merging), lopsided (the wave, probing), both beyond 4096 slots (still the wave: nothing is deferred there)"""
    ln = range_slots(states, n)
    short = np.nonzero((ln > 0) & (ln <= LANE_SLOTS))[0]
    edge = np.nonzero(ln == LANE_SLOTS)[0]
    over = np.nonzero((ln > LANE_SLOTS) & (ln <= LANE_SLOTS + 8))[0]
    mid = np.nonzero((ln >= 300) & (ln <= WAVE_SLOTS))[0]
    long_ = np.nonzero(ln > WAVE_SLOTS)[0]
    assert len(short) >= 20 and len(over) >= 2 and len(mid) >= 5 and len(long_) >= HUBS and set(hubs) <= set(long_.tolist())
    groups = {
        "lane": [(int(x), int(y)) for x, y in zip(rng.choice(short, 60), rng.choice(short, 60))] + [(int(x), int(x)) for x in edge[:4]],
        "over": [(int(x), int(y)) for x in over[:6] for y in rng.choice(short, 4)] + [(int(y), int(x)) for x in over[:6] for y in rng.choice(short, 2)]
                + [(int(x), int(y)) for x in over[:4] for y in over[:4]],
        "lopsided": [(int(x), int(y)) for x in mid[-6:] for y in rng.choice(short, 4)] + [(int(y), int(x)) for x in long_[:6] for y in rng.choice(short, 3)]
                    + [(int(x), int(y)) for x in long_[:4] for y in mid[ln[mid] < ln[long_].min() // 9][:3]],
        "long": [(int(x), int(y)) for x in long_[:6] for y in long_[-4:]] + [(int(long_[0]), int(long_[0]))],
    }
    want_route = {"lane": {"lane"}, "over": {"wave_merge", "wave_probe"}, "lopsided": {"wave_probe"}, "long": {"wave_merge"}}
    for g, prs in groups.items():
        for x, y in prs:
            la, lb = int(ln[x]), int(ln[y])
            route = "lane" if la <= LANE_SLOTS and lb <= LANE_SLOTS else wave_route(la, lb)
            assert route in want_route[g], (g, x, y, la, lb, route)
    assert any(wave_route(int(ln[x]), int(ln[y])) == "wave_merge" for x, y in groups["over"])
    return groups


def check(pp, label):
    n = pp.get_n()
    P = pp.num_partitions()
    states = partition_states(pp)
    for h in pp.isect_hubs:
        node = pp.getNode(h)
        assert node[1] - node[0] - 1 > WAVE_SLOTS + 64, (label, h, node)
    rt = routes(states, n)
    assert_routes(rt, label, P)
    src, dst = global_edges(states)
    want_tri, want_total = model_triangles(src, dst, n)
    tri, total = pp.triangles()
    assert total == want_total and total > n, (label, total, want_total)
    np.testing.assert_array_equal(tri, want_tri, err_msg=f"{label}: tri")
    assert pp.triangles(per_vertex=False) == (None, want_total), label
    groups = pairs_by_route(states, n, pp.isect_hubs, np.random.default_rng(P))
    for g, prs in groups.items():
        a, b = np.array([x for x, _ in prs], np.uint32), np.array([y for _, y in prs], np.uint32)
        want = model_common_neighbours(src, dst, n, a, b)
        assert want.any(), (label, g)
        np.testing.assert_array_equal(pp.common_neighbours(a, b), want, err_msg=f"{label}: common neighbours, {g}")
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):  # nothing written
        assert f0 == f1 and np.array_equal(i0, i1) and np.array_equal(n0, n1), label
    return rt
