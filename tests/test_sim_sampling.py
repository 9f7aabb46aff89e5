"""CPU: ppcsr_sample_neighbours / ppcsr_random_walks / ppcsr_degrees and their pppcsr_ forms on the fiber SIMT emulator
(tests/hostsim), which compiles the engine's own kernel and host source.  States are built by replaying golden fixtures, checked
bit-identical to the oracle, and then sampled: every output is compared exactly with tests/sampling_model.py, which restates the
definition of include/ppcsr.h on the exported states."""
import ctypes

import numpy as np
import pytest

from consumers_model import partition_states
from helpers import golden, load_pkg
from oracle_lib import Oracle, OraclePPPCSR
from sampling_model import NO_VERTEX, mulhi_int, model_degrees, model_sample, model_walks, neighbour_lists
from test_sim_engine import SIM_SO, build_sim
from test_sim_pppcsr_consumers import make as make_pp
from test_sim_queries import make, same_state

EINVAL, EUNSUPPORTED = 1, 4
WAVE_SLOTS = 4096  # kBfsWaveSlots
FANOUTS = (1, 3, 64, 65, 130)
LENGTHS = (1, 5, 40)


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


class One:
    """a PCSR with the calls the checks make on a PPPCSR"""

    def __init__(self, e):
        self.e = e

    def __getattr__(self, name):
        return getattr(self.e, name)

    def num_partitions(self): return 1
    def partition(self, k): return self.e
    def partition_start(self, k): return 0


def queries(n, rng):
    """every vertex, vertices >= n, the sentinel id, repeats; shuffled"""
    q = np.concatenate([np.arange(n), np.arange(n, n + 7), np.array([0xFFFFFFFF]), rng.integers(0, max(n, 1), 40)]).astype(np.uint32)
    return q[rng.permutation(len(q))]


def check(g, label, fanouts=FANOUTS, lengths=LENGTHS, seed=12345):
    """g: a PPPCSR, or One(PCSR).  Everything against the model, exactly; nothing written (states and stats)."""
    n = g.get_n()
    P = g.num_partitions()
    states = partition_states(g)
    stats = [g.partition(k).stats() for k in range(P)]
    rng = np.random.default_rng(n + P)
    q = queries(n, rng)
    for weighted in (False, True):
        for f in fanouts:
            d, v = g.sample_neighbours(q, f, seed=seed + f, weighted=weighted, with_values=True)
            wd, wv = model_sample(states, n, q, f, seed=seed + f, weighted=weighted)
            np.testing.assert_array_equal(d, wd, err_msg=f"{label}: dests, fanout {f}, weighted {weighted}")
            np.testing.assert_array_equal(v, wv, err_msg=f"{label}: values, fanout {f}, weighted {weighted}")
            assert d.shape == (len(q), f)
        np.testing.assert_array_equal(g.sample_neighbours(q, 3, seed=seed + 3, weighted=weighted), model_sample(states, n, q, 3, seed + 3, weighted)[0])
        for length in lengths:
            w = g.random_walks(q, length, seed=seed ^ length, weighted=weighted)
            np.testing.assert_array_equal(w, model_walks(states, n, q, length, seed=seed ^ length, weighted=weighted),
                                          err_msg=f"{label}: walks of {length}, weighted {weighted}")
    deg, wsum = g.degrees(), g.degrees(weighted=True)
    want_deg, want_wsum = model_degrees(states, n)
    np.testing.assert_array_equal(deg, want_deg, err_msg=f"{label}: degrees")
    np.testing.assert_array_equal(wsum, want_wsum, err_msg=f"{label}: weighted degrees")
    assert deg.dtype == np.uint32 and wsum.dtype == np.uint64
    rows, dests, values = neighbour_lists(states, n)  # the model's two definitions agree: by range and by source
    np.testing.assert_array_equal(np.diff(rows), want_deg, err_msg=f"{label}: |L(v)| by range")
    grows, gdests, _ = g.gather_neighbourhoods(np.arange(n, dtype=np.uint32))  # and the gather's rows, restricted to dests < n
    keep = (gdests >= 0) & (gdests.astype(np.int64) < n)
    row_of = np.repeat(np.arange(n), np.diff(grows.astype(np.int64)))
    np.testing.assert_array_equal(deg, np.bincount(row_of[keep], minlength=n), err_msg=f"{label}: degrees against the gather")
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(g)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [g.partition(k).stats() for k in range(P)], label
    return states


def replay(lib, name, upto=None):
    g = golden(name)
    n, lock = int(g["n"]), bool(int(g["lock_search"]))
    e, o = make(lib, n, lock), Oracle(n, lock_search=lock)
    ops = g["ops"][: upto]
    e.apply(ops)
    o.apply(ops)
    same_state(e, o, name)
    return e, o


def test_sim_mulhi_wrapper(lib):
    """the wave layer's 128-bit product against Python ints"""
    e = make(lib, 4)
    edge = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1]
    a = np.array([x for x in edge for _ in edge], np.uint64)
    b = np.array([y for _ in edge for y in edge], np.uint64)
    got = e.debug_mulhi(a, b)
    assert [int(x) for x in got] == [mulhi_int(x, y) for x, y in zip(a, b)]
    assert len(e.debug_mulhi([], [])) == 0


def test_sim_sampling_random_fixture(lib):
    e, _ = replay(lib, "random_2e4_n1000")
    states = check(One(e), "random_2e4_n1000")
    rows, _, _ = neighbour_lists(states, 1000)
    assert np.diff(rows).max() > 10


def test_sim_sampling_gaps_after_deletes(lib):
    """mixed_existing_80k_n2000: 25 000 deletes of stored edges leave gaps inside the ranges"""
    e, _ = replay(lib, "mixed_existing_80k_n2000")
    items, nodes = e.state()
    lens = nodes[:, 1].astype(np.int64) - nodes[:, 0] - 1
    assert (items[:, 2] != 0).sum() - len(nodes) < 0.7 * lens.sum()  # (a good share of every range is null)
    check(One(e), "mixed_existing_80k_n2000", fanouts=(1, 65), lengths=(5,))


def test_sim_sampling_hub_fixture(lib):
    """hub_1e4_insert_then_delete, before and after its deletes: one range beyond kBfsWaveSlots (most of its dests lie beyond n:
    chunks of measure 0)"""
    g = golden("hub_1e4_insert_then_delete")
    e, o = replay(lib, "hub_1e4_insert_then_delete", 10000)
    _, nodes = e.state()
    assert (nodes[:, 1].astype(np.int64) - nodes[:, 0] - 1).max() > WAVE_SLOTS
    check(One(e), "hub fixture before its deletes")
    e.apply(g["ops"][10000:])
    o.apply(g["ops"][10000:])
    same_state(e, o, "hub fixture")
    check(One(e), "hub fixture after its deletes")


def test_sim_sampling_hub_with_neighbours(lib, streams):
    """a hub whose 6000 dests are all vertices, values up to 2^32 - 2 beside values of 1 (W passes 2^32); 3 partitions too"""
    n = 7000
    rng = np.random.default_rng(3)
    vals = np.where(rng.random(6000) < 0.5, 1, rng.integers(1 << 31, (1 << 32) - 1, 6000)).astype(np.uint32)
    vals[17] = (1 << 32) - 2
    hub = np.stack([np.full(6000, 5, np.uint32), rng.permutation(n)[:6000].astype(np.uint32), vals], 1)
    tail = np.array([[6, 5, 3], [7, 7, 9], [8, n + 3, 1], [6999, 5, 1], [6999, 0, (1 << 32) - 2]], np.uint32)
    mids = [np.stack([np.full(m, v, np.uint32), rng.permutation(n)[:m].astype(np.uint32), rng.integers(1, 1 << 20, m).astype(np.uint32)], 1)
            for v, m in ((20, 70), (21, 300), (6000, 1500))]  # ordinary vertices of several chunks
    adds = np.concatenate([hub, tail] + mids)
    for P in (1, 3):
        pp = make_pp(lib, n, P)
        pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
        pp.apply(streams.random_stream(n, 3000, seed=8, p_delete=0.2))
        node = pp.getNode(5)
        assert node[1] - node[0] - 1 > WAVE_SLOTS
        for v in (20, 21, 6000):
            node = pp.getNode(v)
            assert 64 < node[1] - node[0] - 1 <= WAVE_SLOTS, (v, node)
        states = check(pp, f"hub P={P}", fanouts=(3, 130), lengths=(5,))
        _, wsum = model_degrees(states, n)
        assert int(wsum[5]) > 1 << 32
        w = pp.random_walks(np.array([6, 6999, 5], np.uint32), 6, seed=1)
        assert (w[:, 1] != NO_VERTEX).all()  # (each of the three has an out-edge)
        pp.close()


def test_sim_sampling_eight_partitions_fixture(lib):
    """pppcsr_p8_n1000 on 8 partitions, bit-identical to the oracle's"""
    g = golden("pppcsr_p8_n1000")
    n = int(g["n"])
    pp, o = make_pp(lib, n, 8), OraclePPPCSR(n, True, 1, 8)
    pp.apply(g["ops"])
    o.apply(g["ops"])
    for k in range(8):
        same_state(pp.partition(k), o.partition(k), f"partition {k}")
    check(pp, "pppcsr_p8_n1000", fanouts=(3, 65), lengths=(5,))
    pp.close()


def test_sim_sampling_eight_partitions_equal_one(lib, streams):
    """one PCSR against P = 8 on the same stream: identical arrays; the device forms of the single engine"""
    n = 600
    ops = streams.random_stream(n, 5000, seed=14, p_delete=0.2)
    ops[:, 2] *= (np.arange(len(ops), dtype=np.uint32) % np.uint32(1000) + np.uint32(1))  # (values: weights that differ)
    pp, one = make_pp(lib, n, 8), make(lib, n)
    pp.apply(ops)
    one.apply(ops)
    rng = np.random.default_rng(8)
    q = queries(n, rng)
    for weighted in (False, True):
        a = pp.sample_neighbours(q, 7, seed=99, weighted=weighted, with_values=True)
        b = one.sample_neighbours(q, 7, seed=99, weighted=weighted, with_values=True)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(pp.random_walks(q, 12, seed=5, weighted=weighted), one.random_walks(q, 12, seed=5, weighted=weighted))
    np.testing.assert_array_equal(pp.degrees(), one.degrees())
    np.testing.assert_array_equal(pp.degrees(weighted=True), one.degrees(weighted=True))
    # the device forms of the single engine (emulator: device memory is host memory)
    d = np.zeros((len(q), 7), np.uint32)
    v = np.zeros((len(q), 7), np.uint32)
    ms = one.sample_neighbours_device(q.ctypes.data, len(q), 7, d.ctypes.data, v.ctypes.data, seed=99, weighted=True, with_ms=True)
    assert ms >= 0.0
    np.testing.assert_array_equal(d, b[0])
    np.testing.assert_array_equal(v, b[1])
    w = np.zeros((len(q), 13), np.uint32)
    one.random_walks_device(q.ctypes.data, len(q), 12, w.ctypes.data, seed=5, weighted=True)
    np.testing.assert_array_equal(w, one.random_walks(q, 12, seed=5, weighted=True))
    pp.close()


def test_sim_sampling_uniform_claims(lib, streams):
    """a small graph with a hub, every wv::uni / wv::bcast of the kernels verified"""
    n = 5000
    adds = np.concatenate([streams.adds(np.full(4500, 11, np.uint32), np.arange(4500, dtype=np.uint32)), streams.random_stream(n, 2000, seed=2)])
    lib.ppcsr_sim_check_uniform(1)
    try:
        for P in (1, 3):
            pp = make_pp(lib, n, P)
            pp.bulk_build_device(adds.ctypes.data, len(adds))
            states = partition_states(pp)
            q = np.array([11, 0, 11, n, 4999, 12, 11], np.uint32)
            for weighted in (False, True):
                np.testing.assert_array_equal(pp.sample_neighbours(q, 70, seed=3, weighted=weighted), model_sample(states, n, q, 70, 3, weighted)[0])
                np.testing.assert_array_equal(pp.random_walks(q, 4, seed=3, weighted=weighted), model_walks(states, n, q, 4, 3, weighted))
            np.testing.assert_array_equal(pp.degrees(), model_degrees(states, n)[0])
            pp.close()
    finally:
        lib.ppcsr_sim_check_uniform(0)


def test_sim_sampling_empty_graph_and_seeds(lib, streams):
    e = make(lib, 50)
    q = np.arange(60, dtype=np.uint32)
    assert np.all(e.sample_neighbours(q, 4) == NO_VERTEX)
    w = e.random_walks(q, 3)
    assert np.all(w[:50, 0] == np.arange(50)) and np.all(w[50:, 0] == NO_VERTEX) and np.all(w[:, 1:] == NO_VERTEX)
    assert not e.degrees().any() and not e.degrees(weighted=True).any()
    assert e.sample_neighbours([], 4).shape == (0, 4) and e.random_walks([], 4).shape == (0, 5)
    e.apply(streams.random_stream(50, 800, seed=4))
    a, b, c = e.sample_neighbours(q, 9, seed=1), e.sample_neighbours(q, 9, seed=1), e.sample_neighbours(q, 9, seed=2)
    np.testing.assert_array_equal(a, b)
    assert (a != c).any()
    assert (e.random_walks(q, 9, seed=1) != e.random_walks(q, 9, seed=2)).any()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_sampling_refusals(lib, streams, P):
    """every refusal returns its status before anything is launched (outputs untouched), and the engine stays usable"""
    pkg = load_pkg()
    n = 400
    pp = make_pp(lib, n, P)
    pp.apply(streams.random_stream(n, 3000, seed=6))
    L, e = pp.L, pp.partition(P - 1)
    q = np.array([1, 2, 3], np.uint32)
    out = np.full(3 * 4, 77, np.uint32)
    val = np.full(3 * 4, 77, np.uint32)
    deg = np.full(n, 77, np.uint32)
    Q, O, V = q.ctypes.data, out.ctypes.data, val.ctypes.data
    samplers = [(L.pppcsr_sample_neighbours, pp.h), (L.ppcsr_sample_neighbours, e.h), (L.ppcsr_sample_neighbours_device, e.h)]
    walkers = [(L.pppcsr_random_walks, pp.h), (L.ppcsr_random_walks, e.h), (L.ppcsr_random_walks_device, e.h)]
    for fn, h in samplers:
        assert fn(None, Q, 3, 4, 0, 0, O, V, None) == EINVAL
        assert fn(h, None, 3, 4, 0, 0, O, V, None) == EINVAL
        assert fn(h, Q, 3, 4, 0, 0, None, V, None) == EINVAL
        assert fn(h, Q, 3, 0, 0, 0, O, V, None) == EINVAL
        assert fn(h, Q, 3, 4, 0, 2, O, V, None) == EINVAL and "flags" in L.ppcsr_last_error().decode()
        assert fn(h, None, 0, 4, 0, 0, None, None, None) == 0  # k == 0: nothing to read or write
    for fn, h in walkers:
        assert fn(None, Q, 3, 3, 0, 0, O, None) == EINVAL
        assert fn(h, None, 3, 3, 0, 0, O, None) == EINVAL
        assert fn(h, Q, 3, 3, 0, 0, None, None) == EINVAL
        assert fn(h, Q, 3, 0, 0, 0, O, None) == EINVAL
        assert fn(h, Q, 3, 3, 0, 0x80000000, O, None) == EINVAL
        assert fn(h, None, 0, 3, 0, 0, None, None) == 0
    for fn, h in ((L.pppcsr_degrees, pp.h), (L.ppcsr_degrees, e.h)):
        assert fn(h, None, None, None) == EINVAL
        assert fn(None, deg.ctypes.data, None, None) == EINVAL
    assert np.all(out == 77) and np.all(val == 77) and np.all(deg == 77)
    # the sequential regime: sampling refused, degrees answered
    states = partition_states(pp)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    for fn, h in samplers:
        assert fn(h, Q, 3, 4, 0, 0, O, V, None) == EUNSUPPORTED
        assert "sequential regime" in L.ppcsr_last_error().decode()
    for fn, h in walkers:
        assert fn(h, Q, 3, 3, 0, 0, O, None) == EUNSUPPORTED
    assert np.all(out == 77) and np.all(val == 77)
    with pytest.raises(pkg.PpcsrError):
        pp.sample_neighbours(q, 2)
    np.testing.assert_array_equal(pp.degrees(), model_degrees(states, n)[0])
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        np.testing.assert_array_equal(i0, i1)
        np.testing.assert_array_equal(n0, n1)
    pp.apply(streams.random_stream(n, 600, seed=5, p_delete=0.3))  # (routes ops to every partition: the range check runs)
    assert e.stats()["narrow"] == 1
    check(pp, f"P={P} after the regime", fanouts=(3,), lengths=(5,))
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    assert L.pppcsr_sample_neighbours(loc.h, Q, 3, 4, 0, 0, O, V, None) == EINVAL and "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_random_walks(loc.h, Q, 3, 3, 0, 0, O, None) == EINVAL
    assert L.pppcsr_degrees(loc.h, deg.ctypes.data, None, None) == EINVAL
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one)
    pp.close()
