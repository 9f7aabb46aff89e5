"""CPU: ppcsr_path_counts / ppcsr_betweenness and their pppcsr_ forms on the fiber SIMT emulator (tests/hostsim), which compiles
the engine's own kernel and host source.  Levels and path counts are checked exactly, betweenness within the bound derived in
include/ppcsr.h (tests/betweenness_model.py: tolerance), against Brandes' algorithm on Python integers and Fractions built from
the exported partition states."""
import ctypes

import numpy as np
import pytest

from betweenness_model import assert_bc, csr, dag, diamond_chain, model_betweenness, model_path_counts, non_integers, sigma_as_f64, tolerance
from consumers_model import global_edges, last_slot_free, partition_states
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim
from test_sim_paths import _best_start, seams
from test_sim_pppcsr_consumers import make, mixed_stream, starts_of, tune

EINVAL, EUNSUPPORTED = 1, 4
NO_LEVEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


def check(pp, sources, label, exact=True, hard=False, counts_from=None):
    """path_counts from `counts_from` (default: every source) exactly, betweenness from `sources` within the bound; nothing
    written (states and stats).  hard: the conditions that keep the test from passing on an easy input, from the model alone"""
    n = pp.get_n()
    states = partition_states(pp)
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    src, dst = global_edges(states)
    any_above_one = False
    for s in sources if counts_from is None else counts_from:
        lv, sg, h = model_path_counts(src, dst, n, s)
        assert h["max_sigma"] < 2 ** 53, (label, h)
        any_above_one = any_above_one or h["max_sigma"] > 1
        got_lv, got_sg = pp.path_counts(s)
        np.testing.assert_array_equal(got_lv, lv, err_msg=f"{label}: levels from {s}")
        np.testing.assert_array_equal(got_sg, sigma_as_f64(sg), err_msg=f"{label}: sigma from {s}")
    want, info = model_betweenness(src, dst, n, sources, exact)
    if hard:
        assert 4 * info["reached"] >= n, (label, info)
        assert info["widest"] >= max(64, n // 256), (label, info)  # both streaming passes run
        assert info["D"] >= 3 and any_above_one, (label, info)
        assert non_integers(want) >= 1, label
    got = pp.betweenness(sources)
    worst = assert_bc(got, want, tolerance(info["D"], info["dmax"], len(sources), against_fp64=not exact), label)
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return got, want, info, worst


@pytest.mark.parametrize("P", [1, 3, 8])
def test_sim_betweenness_model(lib, streams, P):
    """the mixed stream of test_sim_paths_model (deletes, duplicate adds, destinations >= n), add_node twice, tail edges;
    sources at the partition seams, the busiest vertex, an isolated vertex and the added vertex; again after a repartition to
    balanced_starts"""
    n = 1200
    pp = make(lib, n, P)
    ops = mixed_stream(streams, n, seed=40 + P)
    tail = np.array([[n, 3, 2], [n, 5, 1], [7, n, 3], [n + 5, 1, 1]], np.uint32)  # vertex n + 1 stays isolated
    pp.apply(ops[: len(ops) // 2])
    pp.apply(ops[len(ops) // 2:])
    pp.add_node()
    pp.add_node()
    pp.apply(tail)
    busiest = _best_start(pp)
    sources = starts_of(pp, n + 1) + seams(pp) + [busiest, n]
    got, want, info, _ = check(pp, sources, f"P={P}", hard=True)
    assert got[n + 1] == 0.0 and want[n + 1] == 0  # isolated: on no path
    pp.repartition(pp.balanced_starts())
    tune(pp)
    check(pp, starts_of(pp, n + 1) + seams(pp) + [busiest, n], f"P={P} repartitioned", hard=True)
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_betweenness_deferred_hub(lib, streams, P):
    """the bulk-built hub graph of test_sim_paths_model: a 5000-edge hub whose slot range no single wave walks, as a source
    (level 0) and two levels below another source — deferred to the streaming pass in both sweeps"""
    n, m = 1200, 5000
    hub = 3 if P == 1 else 2 * n // P + 1
    rng = np.random.default_rng(P)
    adds = np.concatenate([streams.adds(np.full(m, hub, np.uint32), rng.permutation(m + 500)[:m].astype(np.uint32)),
                           streams.adds(*streams.rmat_edges_folded(n, 11, 2000, seed=9))])
    pp = make(lib, n, P)
    pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
    node = pp.getNode(hub)
    assert node[1] - node[0] > 4096
    src, dst = global_edges(partition_states(pp))
    back, _, _ = dag(*csr(dst[dst < n], src[dst < n], n), n, hub)  # levels of the reversed graph: distances TO the hub
    above = next(v for v in np.nonzero(back == 2)[0].tolist() if model_path_counts(src, dst, n, v)[2]["D"] >= 3)
    assert model_path_counts(src, dst, n, above)[0][hub] == 2
    _, want, info, _ = check(pp, [hub, above], f"hub P={P}")
    assert want[hub] > 0 and info["dmax"] >= 1000
    pp.close()


@pytest.mark.parametrize("P", [1, 4])
def test_sim_betweenness_counts_beyond_64_bits(lib, P):
    """70 diamonds: 2^70 shortest paths reach the end, 140 levels deep — every count is a power of two, so path_counts stays
    exact beyond 2^53"""
    n, links = 300, 70
    ops, a = diamond_chain(n, links, seed=P)
    pp = make(lib, n, P)
    pp.apply(ops[np.random.default_rng(5).permutation(len(ops))])
    src, dst = global_edges(partition_states(pp))
    lv, sg, h = model_path_counts(src, dst, n, int(a[0]))
    assert h["D"] == 140 and sg[a[-1]] == 2 ** 70 == h["max_sigma"]
    got_lv, got_sg = pp.path_counts(int(a[0]))
    np.testing.assert_array_equal(got_lv, lv)
    np.testing.assert_array_equal(got_sg, sigma_as_f64(sg))
    assert got_sg[a[-1]] == 2.0 ** 70
    sources = [int(a[0]), int(a[35]), int(a[-1])]
    want, info = model_betweenness(src, dst, n, sources, exact=True)
    assert info["D"] == 140 and info["dmax"] == 2
    got = pp.betweenness(sources)
    assert_bc(got, want, tolerance(140, 2, len(sources)), f"diamonds P={P}")
    assert want[a[1]] == 3 * 69 and got[a[1]] == float(want[a[1]])  # (from a_0: a_2 .. a_70 and the 2 x 69 vertices between them)
    pp.close()


def test_sim_betweenness_conventions(lib):
    """only a -> b -> c: b lies between a and c in one direction; a repeated source counts twice; no source, no score;
    endpoints get nothing"""
    pp = make(lib, 20, 2)
    a, b, c = 13, 4, 17
    pp.apply(np.array([[a, b, 5], [b, c, 9]], np.uint32))
    want = np.zeros(20)
    want[b] = 1.0
    np.testing.assert_array_equal(pp.betweenness([a]), want)
    np.testing.assert_array_equal(pp.betweenness([c]), np.zeros(20))
    np.testing.assert_array_equal(pp.betweenness([b]), np.zeros(20))
    np.testing.assert_array_equal(pp.betweenness([a, a]), 2 * want)
    np.testing.assert_array_equal(pp.betweenness([a, c, b, a]), 2 * want)
    np.testing.assert_array_equal(pp.betweenness([]), np.zeros(20))
    np.testing.assert_array_equal(pp.betweenness(np.arange(20)), want)
    lv, sg = pp.path_counts(a)
    assert (lv[a], lv[b], lv[c]) == (0, 1, 2) and np.count_nonzero(lv == NO_LEVEL) == 17
    assert sg[a] == sg[b] == sg[c] == 1.0 and sg.sum() == 3.0
    lv, sg = pp.path_counts(c)
    assert lv[c] == 0 and sg[c] == 1.0 and sg.sum() == 1.0
    pp.close()


def test_sim_betweenness_invariant(lib, streams):
    """P = 1, 2, 4, 8 on one stream, and one graph before and after a repartition with an empty partition: path_counts
    equal, betweenness within the bound of the model each; P = 1 equals the partition's own engine calls, under the same rule"""
    n = 1000
    ops = mixed_stream(streams, n, seed=5)
    sources = [0, 333, 999, n // 2 + 1, int(ops[0, 0])]
    counts, want, tol = [], None, None
    for P in (1, 2, 4, 8):
        pp = make(lib, n, P)
        pp.apply(ops)
        assert all(last_slot_free(i) for _, i, _ in partition_states(pp)), P
        if want is None:
            want, info = model_betweenness(*global_edges(partition_states(pp)), n, sources, exact=True)
            tol = tolerance(info["D"], info["dmax"], len(sources))
            assert 4 * info["reached"] >= n and non_integers(want) >= 1
        counts.append([pp.path_counts(s) for s in sources])
        assert_bc(pp.betweenness(sources), want, tol, f"P={P}")
        if P == 1:
            e = pp.partition(0)
            for s, (lv, sg) in zip(sources, counts[0]):
                got_lv, got_sg, ms = e.path_counts(s, with_ms=True)
                np.testing.assert_array_equal(got_lv, lv)
                np.testing.assert_array_equal(got_sg, sg)
                assert ms >= 0.0
            assert_bc(e.betweenness(sources), want, tol, "the partition's own call")
        if P == 4:
            pp.repartition(np.array([0, 100, 100, 700], np.uint64))  # (an empty partition contributes nothing)
            tune(pp)
            assert all(last_slot_free(i) for _, i, _ in partition_states(pp))
            counts.append([pp.path_counts(s) for s in sources])
            assert_bc(pp.betweenness(sources), want, tol, "empty partition")
        pp.close()
    for other in counts[1:]:
        for (lv, sg), (lv0, sg0) in zip(other, counts[0]):
            np.testing.assert_array_equal(lv, lv0)
            np.testing.assert_array_equal(sg, sg0)


def test_sim_betweenness_uniform(lib, streams):
    """the plain folded RMAT graph (n = 1200, scale 11, 3000 edges, seed 41), 21 sources, with every wv::uni / wv::bcast of
    the kernels verified"""
    n = 1200
    s, d = streams.rmat_edges_folded(n, 11, 3000, seed=41)
    lib.ppcsr_sim_check_uniform(1)
    try:
        pp = make(lib, n, 3)
        pp.apply(streams.adds(s, d))
        busiest = _best_start(pp)
        sources = [busiest] + list(range(0, n, 60))
        assert len(sources) == 21
        _, want, info, worst = check(pp, sources, "uniform", hard=True, counts_from=[busiest, 0])
        assert info["D"] >= 5 and info["dmax"] >= 100
        pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


@pytest.mark.parametrize("P", [1, 3])
def test_sim_betweenness_answers_in_the_sequential_regime(lib, streams, P):
    """narrow == 0 on one partition: the call is not refused (it intersects nothing) and matches the model"""
    n = 500
    pp = make(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 9, 6000, seed=23)
    adds = streams.adds(s, d)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    e = pp.partition(P - 1)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    tri = np.empty(n, np.uint64)
    assert pp.L.pppcsr_triangles(pp.h, tri.ctypes.data, None, None) == EUNSUPPORTED  # (the regime is the one triangles refuses)
    check(pp, [_best_start(pp), 0, n - 1], f"sequential P={P}")
    lv, sg = e.path_counts(0)
    assert len(lv) == len(sg) == e.get_n()
    assert len(e.betweenness([0])) == e.get_n()
    assert e.stats()["narrow"] == 0
    pp.close()


def test_betweenness_model_against_networkx(lib, streams):
    """the model itself against networkx.betweenness_centrality on a directed graph, all sources"""
    nx = pytest.importorskip("networkx")
    n = 300
    pp = make(lib, n, 3)
    pp.apply(mixed_stream(streams, n, seed=8))
    src, dst = global_edges(partition_states(pp))
    ok = dst < n
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(src[ok].tolist(), dst[ok].tolist()))
    ref = nx.betweenness_centrality(g, normalized=False)
    ref = np.array([ref[v] for v in range(n)], np.float64)
    sources = np.arange(n)
    exact, info = model_betweenness(src, dst, n, sources, exact=True)
    fp64, info2 = model_betweenness(src, dst, n, sources, exact=False)
    assert info == {**info2, "max_sigma": int(info2["max_sigma"])}
    tol = tolerance(info["D"], info["dmax"], n, against_fp64=True)
    assert_bc(ref, fp64, tol, "networkx against the fp64 model")
    assert_bc(fp64, exact, tolerance(info["D"], info["dmax"], n), "the fp64 model against the exact one")
    assert non_integers(exact) >= 1 and info["D"] >= 3
    assert_bc(pp.betweenness(sources), exact, tolerance(info["D"], info["dmax"], n), "device")
    pp.close()


def test_sim_betweenness_errors(lib, streams):
    pkg = load_pkg()
    n = 300
    pp = make(lib, n, 3)
    pp.apply(streams.random_stream(n, 500, seed=1))
    L, h = pp.L, pp.h
    e = pp.partition(0)
    lv = np.empty(n, np.uint32)
    sg = np.empty(n, np.float64)
    bc = np.empty(n, np.float64)
    ms = ctypes.c_double()
    for pc, bt, hh, m in ((L.pppcsr_path_counts, L.pppcsr_betweenness, h, n), (L.ppcsr_path_counts, L.ppcsr_betweenness, e.h, e.get_n())):
        src_ok = np.array([0, m - 1, 0], np.uint32)
        src_bad = np.array([0, m, 1], np.uint32)
        assert pc(hh, m, lv.ctypes.data, sg.ctypes.data, ctypes.byref(ms)) == EINVAL
        assert pc(hh, 0xFFFFFFFF, lv.ctypes.data, sg.ctypes.data, None) == EINVAL
        assert pc(hh, 0, None, None, None) == EINVAL
        assert pc(None, 0, lv.ctypes.data, sg.ctypes.data, None) == EINVAL
        assert pc(hh, m - 1, lv.ctypes.data, None, None) == 0  # either output may be NULL, device_ms may be NULL
        assert pc(hh, m - 1, None, sg.ctypes.data, None) == 0
        assert pc(hh, 0, lv.ctypes.data, sg.ctypes.data, ctypes.byref(ms)) == 0 and ms.value >= 0.0
        assert lv[0] == 0 and sg[0] == 1.0
        assert bt(None, src_ok.ctypes.data, 3, bc.ctypes.data, None) == EINVAL
        assert bt(hh, src_ok.ctypes.data, 3, None, None) == EINVAL
        assert bt(hh, None, 3, bc.ctypes.data, None) == EINVAL
        bc[:] = 77.0
        assert bt(hh, src_bad.ctypes.data, 3, bc.ctypes.data, None) == EINVAL
        assert "out of range" in L.ppcsr_last_error().decode() and np.all(bc == 77.0)  # refused before anything ran
        assert bt(hh, src_bad.ctypes.data, 1, bc.ctypes.data, None) == 0  # (only the first source is read)
        assert bt(hh, None, 0, bc.ctypes.data, None) == 0 and not bc[:m].any() and np.all(bc[m:] == 77.0)
        assert bt(hh, src_ok.ctypes.data, 3, bc.ctypes.data, ctypes.byref(ms)) == 0 and ms.value >= 0.0
    with pytest.raises(pkg.PpcsrError):
        pp.path_counts(n)
    with pytest.raises(pkg.PpcsrError):
        pp.betweenness([0, n])
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_path_counts(loc.h, 100, lv.ctypes.data, sg.ctypes.data, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_betweenness(loc.h, np.array([100], np.uint32).ctypes.data, 1, bc.ctypes.data, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    # (EUNSUPPORTED — partitions on several devices — needs a second device: the emulator has one)
    pp.close()
