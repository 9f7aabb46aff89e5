"""GPU: ppcsr_path_counts / ppcsr_betweenness and their pppcsr_ forms on MI355X, all partitions on one device.  Levels and
path counts are compared exactly, betweenness within the bound derived in include/ppcsr.h (tests/betweenness_model.py:
tolerance — twice the bound against the fp64 model, which carries the same error itself), from the exported partition states."""
import numpy as np
import pytest

from betweenness_model import assert_bc, diamond_chain, model_betweenness, model_path_counts, non_integers, sigma_as_f64, tolerance
from consumers_model import global_edges, partition_states
from helpers import load_pkg

pytestmark = pytest.mark.gpu

WAVE_SLOTS = 4096  # longest slot range one wave walks on its own
STREAM_GRID_SLOTS = 8192 * 4 * 256  # slots one step of the streaming grids covers once they stop growing: 8192 workgroups of 4 waves, 4 chunks of 64 slots each


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()
    return p


def busiest(src, dst, n, but=()):
    deg = np.bincount(src[dst < n], minlength=n)
    deg[list(but)] = 0
    return int(deg.argmax())


def check_fp64(objs, edges, sources, label, count_sources):
    """every object of `objs` (same edge set) against one fp64 model: path_counts exactly, betweenness within the bound"""
    src, dst, n = edges
    counts = {}
    want, info = model_betweenness(src, dst, n, sources, exact=False, counts=counts)
    assert info["max_sigma"] < 2.0 ** 53, (label, info)
    tol = tolerance(info["D"], info["dmax"], len(sources), against_fp64=True)
    assert set(count_sources) <= set(counts)
    for name, g in objs:
        for s in count_sources:
            lv, sg = counts[s]
            got_lv, got_sg = g.path_counts(s)
            np.testing.assert_array_equal(got_lv, lv, err_msg=f"{label} {name}: levels from {s}")
            np.testing.assert_array_equal(got_sg, sg, err_msg=f"{label} {name}: sigma from {s}")
        worst = assert_bc(g.betweenness(sources), want, tol, f"{label} {name}")
        print(f"{label} {name}: D={info['D']} dmax={info['dmax']} widest={info['widest']} reached={info['reached']} "
              f"max sigma={info['max_sigma']:.3g} worst relative error {worst:.3g} bound {tol:.3g}")
    return want, info


def test_betweenness_model_rmat14(pkg, streams):
    """n = 2^14 on 8 partitions and on one PCSR: a 120 K-edge RMAT core and a 6000-edge hub, then a mixed stream (deletes,
    duplicate adds, destinations >= n); 16 sources with the hub and the busiest other vertex among them"""
    n, P, hub = 1 << 14, 8, 9001
    s, d = streams.rmat_edges(14, 120_000, seed=71)
    rng = np.random.default_rng(7)
    core = np.concatenate([streams.adds(s, d), streams.adds(np.full(6000, hub, np.uint32), rng.permutation(n)[:6000].astype(np.uint32))])
    s2, d2 = streams.rmat_edges(14, 20_000, seed=72)
    mixed = streams.mixed_existing_stream(core[:120_000], streams.adds(s2, d2 + np.uint32(3)), seed=73)
    mixed = mixed[mixed[:, 0] != hub]  # (the hub keeps its range)
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    one = pkg.PCSR(n)
    for g in (pp, one):
        g.apply(core)
        g.apply(mixed)
    states = partition_states(pp)
    src, dst = global_edges(states)
    items, nodes = one.state()
    s1, d1 = global_edges([(0, items, nodes)])
    assert np.array_equal(src, s1) and np.array_equal(dst, d1)
    for g in (pp, one):
        beginning, end, _ = g.getNode(hub)
        assert end - beginning > WAVE_SLOTS
    top = busiest(src, dst, n, but=[hub])
    sources = [hub, top, 0, n - 1, n // P, n // P - 1] + [int(x) for x in rng.integers(0, n, 10)]
    assert len(sources) == 16
    want, info = check_fp64([("P=8", pp), ("PCSR", one)], (src, dst, n), sources, "rmat14", [hub, top, n // P])
    assert info["widest"] >= max(64, n // 256) and 4 * info["reached"] >= n and info["D"] >= 3, info
    assert non_integers(want) >= 1 and info["dmax"] >= 6000
    for (_, i0, n0), (_, i1, n1) in zip(states, partition_states(pp)):  # nothing written
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1)
    pp.close()


@pytest.mark.parametrize("P", [1, 4])
def test_betweenness_counts_beyond_64_bits(pkg, P):
    """70 two-wide diamonds: 2^70 paths, 140 levels; path_counts exact, betweenness within the bound of the Fraction model"""
    n, links = 300, 70
    ops, a = diamond_chain(n, links, seed=P)
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    pp.apply(ops[np.random.default_rng(5).permutation(len(ops))])
    src, dst = global_edges(partition_states(pp))
    lv, sg, h = model_path_counts(src, dst, n, int(a[0]))
    assert h["D"] == 140 and sg[a[-1]] == 2 ** 70
    got_lv, got_sg = pp.path_counts(int(a[0]))
    np.testing.assert_array_equal(got_lv, lv)
    np.testing.assert_array_equal(got_sg, sigma_as_f64(sg))
    sources = [int(a[0]), int(a[35]), int(a[-1])]
    want, info = model_betweenness(src, dst, n, sources, exact=True)
    assert info["D"] == 140 and info["dmax"] == 2
    got = pp.betweenness(sources)
    worst = assert_bc(got, want, tolerance(140, 2, len(sources)), f"diamonds P={P}")
    print(f"diamonds P={P}: worst relative error {worst:.3g} bound {tolerance(140, 2, 3):.3g}")
    assert want[a[1]] == 3 * 69 and got[a[1]] == 207.0
    pp.close()


def test_betweenness_follows_batches(pkg, streams):
    """3 rounds of: apply a batch, then path_counts and betweenness from four sources against the model (scale 14)"""
    n, P = 1 << 14, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges(14, 60_000, seed=61)
    pp.apply(streams.adds(s, d))
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 20_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 10_000, seed=80 + r, p_delete=0.5)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        src, dst = global_edges(partition_states(pp))
        top = busiest(src, dst, n)
        check_fp64([("P=8", pp)], (src, dst, n), [top, r * 1000 + 1, n - 1 - r, 4096 + r], f"round {r}", [top])
    pp.close()


def test_betweenness_grid_stride_seam(pkg, streams):
    """one bulk-built array of more slots than one step of the streaming grids covers (they stop growing at 8192
    workgroups), so that their grid-stride loops take a second step: n = 2^19, 6.2 M uniform random edges (bulk build
    doubles the array while n + E + 1 >= 3/4 of its slots: 2^24 slots) and a hub of 2^16, one source; the model is numpy
    throughout (np.add.at per level)"""
    n, hub = 1 << 19, 77
    rng = np.random.default_rng(9)
    s, d = rng.integers(0, n, 6_200_000).astype(np.uint32), rng.integers(0, n, 6_200_000).astype(np.uint32)
    adds = np.concatenate([streams.adds(s, d), streams.adds(np.full(1 << 16, hub, np.uint32), rng.permutation(n)[: 1 << 16].astype(np.uint32))])
    one = pkg.PCSR(n)
    one.bulk_build(adds)
    items, nodes = one.state()
    assert len(items) > STREAM_GRID_SLOTS, len(items)
    beginning, end, _ = one.getNode(hub)
    assert end - beginning > WAVE_SLOTS
    src, dst = global_edges([(0, items, nodes)])
    want, info = check_fp64([("PCSR", one)], (src, dst, n), [hub], "seam", [hub])
    assert info["widest"] >= n // 256 and 4 * info["reached"] >= n and non_integers(want) >= 1, info
