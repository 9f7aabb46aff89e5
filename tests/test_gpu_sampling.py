"""GPU: ppcsr_sample_neighbours / ppcsr_random_walks / ppcsr_degrees and their pppcsr_ forms on MI355X, every output compared
exactly with tests/sampling_model.py (the definition of include/ppcsr.h restated on the exported states): a hand-built graph
with one vertex per case the kernels tell apart (tests/sampling_graphs.py), more queries than the grid has waves, a scale-14
RMAT graph under mixed batches on one PCSR and on 8 partitions, the device forms on torch tensors, seeds, refusals."""
import numpy as np
import pytest

from consumers_model import partition_states
from helpers import load_pkg
from sampling_graphs import N_VERT, V, WAVE_SLOTS, hand_graph, hand_queries
from sampling_model import NO_VERTEX, mulhi_int, model_degrees, model_sample, model_walks

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()
    return p


def states_of(g):
    return partition_states(g) if hasattr(g, "num_partitions") else [(0, *g.state())]


def stats_of(g):
    return [g.partition(k).stats() for k in range(g.num_partitions())] if hasattr(g, "num_partitions") else [g.stats()]


def same_states(a, b, label):
    for (f0, i0, n0), (f1, i1, n1) in zip(a, b):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)


def check(g, q, fanout, length, label, seed=7, walkers=None, states=None):
    """sample and walk, uniform and weighted, and the degrees, against the model; nothing written"""
    n = g.get_n()
    states = states if states is not None else states_of(g)
    stats = stats_of(g)
    w = q if walkers is None else walkers
    out = {}
    for weighted in (False, True):
        d, v = g.sample_neighbours(q, fanout, seed=seed, weighted=weighted, with_values=True)
        wd, wv = model_sample(states, n, q, fanout, seed=seed, weighted=weighted)
        np.testing.assert_array_equal(d, wd, err_msg=f"{label}: dests, weighted {weighted}")
        np.testing.assert_array_equal(v, wv, err_msg=f"{label}: values, weighted {weighted}")
        walks = g.random_walks(w, length, seed=seed + 1, weighted=weighted)
        np.testing.assert_array_equal(walks, model_walks(states, n, w, length, seed=seed + 1, weighted=weighted),
                                      err_msg=f"{label}: walks, weighted {weighted}")
        out[weighted] = (d, v, walks)
    deg, wsum = model_degrees(states, n)
    np.testing.assert_array_equal(g.degrees(), deg, err_msg=f"{label}: degrees")
    np.testing.assert_array_equal(g.degrees(weighted=True), wsum, err_msg=f"{label}: weighted degrees")
    same_states(states, states_of(g), label)
    assert stats == stats_of(g), label
    return out


@pytest.fixture(scope="module")
def hand(pkg):
    N0 = pkg.PCSR(N_VERT).geometry()[0]
    return hand_graph(N0)


@pytest.mark.parametrize("build", ["bulk_build", "apply"])
def test_hand_built_graph(pkg, hand, build):
    adds, deletes, want = hand
    n = N_VERT
    e = pkg.PCSR(n)
    if build == "bulk_build":
        e.bulk_build(adds)
    else:
        e.apply(adds)
    e.apply(deletes)
    assert e.stats()["narrow"] == 1
    lens = {name: e.getNode(v)[1] - e.getNode(v)[0] - 1 for name, (v, _) in want.items()}
    print(build, "range lengths", lens)
    if build == "bulk_build":  # (the layout of a bulk build is pinned: tests/sampling_graphs.py)
        assert lens["exact"] == WAVE_SLOTS and lens["over"] == WAVE_SLOTS + 1, lens
    assert lens["hub"] > 1 << 18  # past one scan tile of 64-slot chunks
    states = states_of(e)
    deg, wsum = model_degrees(states, n)
    for name, d in (("deg0", 0), ("deg1", 1), ("deg63", 63), ("deg64", 64), ("deg65", 65), ("deg127", 127), ("gone", 0), ("beyond", 0), ("loop", 1)):
        assert deg[V[name]] == d, (name, deg[V[name]])
    assert e.getNode(V["beyond"])[2] == 40  # (num_neighbors is not the live degree)
    assert int(wsum[V["hub"]]) > 1 << 32 and int(wsum[V["deg65"]]) > 1 << 32
    rng = np.random.default_rng(5)
    q = hand_queries(rng, 2000)
    for fanout in (1, 65):
        out = check(e, q, fanout, 6, f"{build} fanout {fanout}", states=states)
    d, _, walks = out[False]
    iq = {name: int(np.nonzero(q == V[name])[0][0]) for name in ("deg0", "gone", "beyond", "loop", "hub")}
    assert np.all(d[iq["deg0"]] == NO_VERTEX) and np.all(d[iq["gone"]] == NO_VERTEX) and np.all(d[iq["beyond"]] == NO_VERTEX)
    assert np.all(d[iq["loop"]] == V["loop"]) and np.all(walks[iq["loop"]] == V["loop"])
    assert np.all(walks[iq["deg0"], 1:] == NO_VERTEX) and walks[iq["deg0"], 0] == V["deg0"]
    assert len(np.unique(d[q == V["hub"]])) > 1000  # (the hub's draws spread over its neighbours)
    e.close()


def test_grid_seam(pkg, hand):
    """more queries and walkers than the per-query grid has waves (16 384 workgroups of 4): 65 537, half of them on the hub"""
    adds, deletes, _ = hand
    e = pkg.PCSR(N_VERT)
    e.bulk_build(adds)
    e.apply(deletes)
    q = hand_queries(np.random.default_rng(6), 65537)
    assert abs(int((q == V["hub"]).sum()) - 32768) < 2000
    check(e, q, 3, 4, "grid seam")
    e.close()


def rmat_batches(streams, n, scale, core, batches, per_batch):
    s, d = streams.rmat_edges_folded(n, scale, core + batches * per_batch, seed=31)
    rng = np.random.default_rng(32)
    val = rng.integers(1, 1 << 20, len(s)).astype(np.uint32)
    ops = np.stack([s, d, val], 1).astype(np.uint32)
    out = [ops[:core]]
    for b in range(batches):
        part = ops[core + b * per_batch: core + (b + 1) * per_batch].copy()
        prev = np.concatenate(out)
        dele = prev[rng.integers(0, len(prev), per_batch // 3)].copy()
        dele[:, 2] = 0
        part[::19] = prev[rng.integers(0, len(prev), len(part[::19]))]  # a duplicate every 19th edge
        part[::19, 2] += np.uint32(1)
        part[5::23, 1] += np.uint32(n)  # destinations beyond the graph
        mix = np.concatenate([part, dele])
        out.append(mix[rng.permutation(len(mix))])
    return out


def test_rmat_batches_one_and_eight_partitions(pkg, streams):
    """scale 14: 60 000 edges, then three mixed batches; after each, seeds and walkers against the model on one PCSR and on
    8 partitions, the two word for word alike, and the device forms on torch tensors equal to the host forms"""
    import torch
    n = 1 << 14
    rng = np.random.default_rng(33)
    one, pp = pkg.PCSR(n), pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=8)
    seeds = rng.integers(0, n + 2, 1 << 15).astype(np.uint32)
    walkers = rng.integers(0, n, 1 << 14).astype(np.uint32)
    for b, ops in enumerate(rmat_batches(streams, n, 14, 60000, 3, 6000)):
        one.apply(ops)
        pp.apply(ops)
        assert one.stats()["narrow"] == 1
        a = check(one, seeds, 10, 20, f"batch {b}, PCSR", seed=b, walkers=walkers)
        # 8 partitions: word for word what the one PCSR gave (which is the model's), its degrees against its own states
        pstates, pstats = partition_states(pp), stats_of(pp)
        for weighted in (False, True):
            d, v = pp.sample_neighbours(seeds, 10, seed=b, weighted=weighted, with_values=True)
            w = pp.random_walks(walkers, 20, seed=b + 1, weighted=weighted)
            for x, y in zip(a[weighted], (d, v, w)):
                np.testing.assert_array_equal(x, y, err_msg=f"batch {b}: one PCSR against 8 partitions")
        deg, wsum = model_degrees(pstates, n)
        np.testing.assert_array_equal(pp.degrees(), deg)
        np.testing.assert_array_equal(pp.degrees(weighted=True), wsum)
        same_states(pstates, partition_states(pp), f"batch {b}, P=8")
        assert pstats == stats_of(pp)
        # device forms
        dq = torch.from_numpy(seeds.view(np.int32)).cuda()
        dd = torch.zeros((len(seeds), 10), dtype=torch.int32, device="cuda")
        dv = torch.zeros((len(seeds), 10), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ms = one.sample_neighbours_device(dq.data_ptr(), len(seeds), 10, dd.data_ptr(), dv.data_ptr(), seed=b, weighted=True, with_ms=True)
        assert ms > 0.0
        np.testing.assert_array_equal(dd.cpu().numpy().view(np.uint32), a[True][0])
        np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), a[True][1])
        one.sample_neighbours_device(dq.data_ptr(), len(seeds), 10, dd.data_ptr(), None, seed=b)
        np.testing.assert_array_equal(dd.cpu().numpy().view(np.uint32), a[False][0])
        dw = torch.from_numpy(walkers.view(np.int32)).cuda()
        do = torch.zeros((len(walkers), 21), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        one.random_walks_device(dw.data_ptr(), len(walkers), 20, do.data_ptr(), seed=b + 1, weighted=True)
        np.testing.assert_array_equal(do.cpu().numpy().view(np.uint32), a[True][2])
    one.close()
    pp.close()


def test_seed_behaviour(pkg, streams):
    """another seed changes the output; the same seed repeats it, across two calls and across snapshot / apply / restore"""
    n = 1 << 12
    e = pkg.PCSR(n)
    e.apply(streams.random_stream(n, 40000, seed=41))
    q = np.arange(n, dtype=np.uint32)
    a = e.sample_neighbours(q, 5, seed=1, with_values=True)
    w = e.random_walks(q, 8, seed=1, weighted=True)
    b = e.sample_neighbours(q, 5, seed=1, with_values=True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert (e.sample_neighbours(q, 5, seed=2) != a[0]).mean() > 0.5
    assert (e.random_walks(q, 8, seed=2, weighted=True)[:, 1:] != w[:, 1:]).mean() > 0.5
    e.snapshot()
    e.apply(streams.random_stream(n, 20000, seed=42, p_delete=0.5))
    assert (e.sample_neighbours(q, 5, seed=1) != a[0]).any()
    e.restore()
    np.testing.assert_array_equal(e.sample_neighbours(q, 5, seed=1), a[0])
    np.testing.assert_array_equal(e.random_walks(q, 8, seed=1, weighted=True), w)
    # 64-bit seeds: the high half counts
    assert (e.sample_neighbours(q, 5, seed=1 << 63) != e.sample_neighbours(q, 5, seed=0)).any()
    states = states_of(e)
    np.testing.assert_array_equal(e.sample_neighbours(q, 5, seed=(1 << 64) - 1), model_sample(states, n, q, 5, seed=(1 << 64) - 1)[0])
    e.close()


def test_mulhi_on_the_device(pkg):
    e = pkg.PCSR(8)
    edge = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1]
    a = np.array([x for x in edge for _ in edge], np.uint64)
    b = np.array([y for _ in edge for y in edge], np.uint64)
    assert [int(x) for x in e.debug_mulhi(a, b)] == [mulhi_int(x, y) for x, y in zip(a, b)]
    e.close()


def test_refusals(pkg, streams):
    """every refusal returns its status with the outputs untouched, and the engine stays usable"""
    n = 1 << 10
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4)
    pp.apply(streams.random_stream(n, 8000, seed=51))
    L, e = pp.L, pp.partition(3)
    q = np.array([1, 2, 3], np.uint32)
    out, val, deg = np.full(12, 77, np.uint32), np.full(12, 77, np.uint32), np.full(n, 77, np.uint32)
    Q, O, Vp = q.ctypes.data, out.ctypes.data, val.ctypes.data
    samplers = [(L.pppcsr_sample_neighbours, pp.h), (L.ppcsr_sample_neighbours, e.h), (L.ppcsr_sample_neighbours_device, e.h)]
    walkers = [(L.pppcsr_random_walks, pp.h), (L.ppcsr_random_walks, e.h), (L.ppcsr_random_walks_device, e.h)]
    for fn, h in samplers:
        assert fn(None, Q, 3, 4, 0, 0, O, Vp, None) == EINVAL
        assert fn(h, None, 3, 4, 0, 0, O, Vp, None) == EINVAL
        assert fn(h, Q, 3, 4, 0, 0, None, Vp, None) == EINVAL
        assert fn(h, Q, 3, 0, 0, 0, O, Vp, None) == EINVAL
        assert fn(h, Q, 3, 4, 0, 2, O, Vp, None) == EINVAL
        assert fn(h, None, 0, 4, 0, 0, None, None, None) == 0
    for fn, h in walkers:
        assert fn(None, Q, 3, 3, 0, 0, O, None) == EINVAL
        assert fn(h, None, 3, 3, 0, 0, O, None) == EINVAL
        assert fn(h, Q, 3, 3, 0, 0, None, None) == EINVAL
        assert fn(h, Q, 3, 0, 0, 0, O, None) == EINVAL
        assert fn(h, Q, 3, 3, 0, 4, O, None) == EINVAL
        assert fn(h, None, 0, 3, 0, 0, None, None) == 0
    for fn, h in ((L.pppcsr_degrees, pp.h), (L.ppcsr_degrees, e.h)):
        assert fn(h, None, None, None) == EINVAL
        assert fn(None, deg.ctypes.data, None, None) == EINVAL
    states = partition_states(pp)
    e.set_option("search_narrow", 0)  # the sequential regime, as the triangle tests reach it
    assert e.stats()["narrow"] == 0
    for fn, h in samplers[:2]:
        assert fn(h, Q, 3, 4, 0, 0, O, Vp, None) == EUNSUPPORTED
        assert "sequential regime" in L.ppcsr_last_error().decode()
    for fn, h in walkers[:2]:
        assert fn(h, Q, 3, 3, 0, 0, O, None) == EUNSUPPORTED
    assert np.all(out == 77) and np.all(val == 77) and np.all(deg == 77)
    np.testing.assert_array_equal(pp.degrees(), model_degrees(states, n)[0])  # (streaming: answered in either regime)
    pp.apply(streams.random_stream(n, 2000, seed=52, p_delete=0.3))  # (the range check runs: the regime ends)
    assert e.stats()["narrow"] == 1
    check(pp, np.arange(n + 3, dtype=np.uint32), 4, 5, "after the regime")
    if L.ppcsr_device_count() >= 2:
        two = pkg.PPPCSR(n, numDomain=2, partitionsPerDomain=1, devices=[0, 1])
        assert L.pppcsr_sample_neighbours(two.h, Q, 3, 4, 0, 0, O, Vp, None) == EUNSUPPORTED
        assert L.pppcsr_random_walks(two.h, Q, 3, 3, 0, 0, O, None) == EUNSUPPORTED
        assert L.pppcsr_degrees(two.h, deg.ctypes.data, None, None) == EUNSUPPORTED
        two.close()
    pp.close()
