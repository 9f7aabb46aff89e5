"""CPU: ppcsr_multi_bfs / pppcsr_multi_bfs on the fiber SIMT emulator (tests/hostsim), which compiles the engine's own kernel
and host source.  States are built by replaying golden fixtures; every output is compared exactly — harmonic bit for bit — with
tests/multibfs_model.py, every levels row with the emulator's own bfs, and the state before with the state after."""
import ctypes
import itertools

import numpy as np
import pytest

from consumers_model import global_edges, partition_states
from helpers import golden, load_pkg
from multibfs_checks import One, check
from multibfs_model import model_multi_bfs
from oracle_lib import OraclePPPCSR
from test_sim_engine import SIM_SO, build_sim
from test_sim_pppcsr_consumers import make as make_pp
from test_sim_queries import same_state
from test_sim_sampling import replay

EINVAL = 1
KS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


def sources_for(g, k, seed):
    """k sources: vertices with an out-edge first (the searches go somewhere), vertex 0 and n - 1, a repeat"""
    n = g.get_n()
    src, dst = global_edges(partition_states(g))
    busy = np.unique(src[dst < n])
    rng = np.random.default_rng(seed)
    pool = busy if len(busy) else np.arange(n)
    s = rng.choice(pool, k, replace=len(pool) < k)
    s[-1] = s[0]
    if k > 3:
        s[1], s[2] = 0, n - 1
    return s.astype(np.uint32)


def test_sim_multibfs_rmat_fixture(lib):
    """rmat12_core60k_mixed40k: union frontiers above and below the threshold of the pass within one call, three groups"""
    e, _ = replay(lib, "rmat12_core60k_mixed40k")
    g = One(e)
    assert not g.debug_multi_bfs_counters().any()  # all zeros before the first call
    m, _, c = check(g, sources_for(g, 130, 1), "rmat12 k=130")
    assert c[0] == 3 and c[2] >= 1 and c[3] >= 1 and c[6] == c[2] + c[3] and c[7] >= c[1], c
    assert max(m["ecc"]) >= 3 and max(m["reached"]) > 1000
    for k in (1, 64):
        check(g, sources_for(g, k, k), f"rmat12 k={k}", bfs_rows=2)


@pytest.fixture(scope="module")
def eight(lib):
    """pppcsr_p8_n1000 on 8 partitions, bit-identical to the oracle's: replayed once (no call writes to it)"""
    g = golden("pppcsr_p8_n1000")
    n = int(g["n"])
    pp, o = make_pp(lib, n, 8), OraclePPPCSR(n, True, 1, 8)
    pp.apply(g["ops"])
    o.apply(g["ops"])
    for q in range(8):
        same_state(pp.partition(q), o.partition(q), f"partition {q}")
    yield pp
    pp.close()


@pytest.mark.parametrize("k", KS)
def test_sim_multibfs_eight_partitions_fixture(eight, k):
    """every k around the group size"""
    _, _, c = check(eight, sources_for(eight, k, 10 + k), f"pppcsr_p8_n1000 k={k}", bfs_rows=3)
    assert c[0] == (k + 63) // 64


def test_sim_multibfs_hub_fixture(lib):
    """hub_1e4_insert_then_delete, before and after its deletes: a range beyond what one wave walks is flagged by the per-vertex
    launch and finished by a pass; most of the hub's destinations lie beyond n"""
    g = golden("hub_1e4_insert_then_delete")
    e, o = replay(lib, "hub_1e4_insert_then_delete", 10000)
    n = e.get_n()
    _, nodes = e.state()
    assert (nodes[:, 1].astype(np.int64) - nodes[:, 0] - 1).max() > 4096
    for k in KS:
        _, _, c = check(One(e), np.arange(k) % n, f"hub fixture k={k}", bfs_rows=None if k == 1 else 3)
        assert c[3] >= 1 and c[4] >= 1, c
    e.apply(g["ops"][10000:])
    o.apply(g["ops"][10000:])
    same_state(e, o, "hub fixture")
    check(One(e), np.arange(65) % n, "hub fixture after its deletes")


def test_sim_multibfs_uniform_claims_and_partitions_agree(lib, streams):
    """a path, a hub and random edges with every wv::uni / wv::bcast of the kernels verified; a PCSR and three partitions with
    the same edges answer word for word alike"""
    n = 5000
    path = streams.adds(np.arange(100, 160, dtype=np.uint32), np.arange(101, 161, dtype=np.uint32))
    hub = streams.adds(np.full(4500, 11, np.uint32), np.arange(4500, dtype=np.uint32))
    adds = np.concatenate([hub, path, streams.random_stream(n, 2000, seed=2)])
    sources = np.array([100, 11, 0, 4999, 100, 130], np.uint32)
    lib.ppcsr_sim_check_uniform(1)
    try:
        got = []
        for P in (1, 3):
            pp = make_pp(lib, n, P)
            pp.bulk_build_device(adds.ctypes.data, len(adds))  # (emulator: device memory is host memory)
            m, g, c = check(pp, sources, f"uniform P={P}", bfs_rows=None)
            assert c[3] >= 1 and c[4] >= 1, c
            got.append(g)
            pp.close()
        for a, b in zip(*got):
            np.testing.assert_array_equal(a, b)
    finally:
        lib.ppcsr_sim_check_uniform(0)


def test_sim_multibfs_closeness_and_lists(lib, streams):
    """closeness = (reached - 1) / far, 0 where far == 0; sources as a list; with_ms"""
    e, _ = replay(lib, "random_2e4_n1000")
    s = [3, 5, 3]
    reached, far, ecc, harm, ms = e.multi_bfs(s, with_ms=True)
    assert ms >= 0.0
    want = np.where(far != 0, (reached.astype(np.float64) - 1.0) / np.maximum(far, 1).astype(np.float64), 0.0)
    np.testing.assert_array_equal(e.closeness(s), want)
    lone = load_pkg().PCSR(4, lib=lib)
    assert e.closeness(s)[0] > 0.0 and lone.closeness([1, 2]).tolist() == [0.0, 0.0]
    assert lone.multi_bfs([2], levels=True)[4].tolist() == [[0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF]]
    r = lone.multi_bfs([], levels=True)
    assert [len(x) for x in r[:4]] == [0, 0, 0, 0] and r[4].shape == (0, 4)


@pytest.mark.parametrize("P", [1, 3])
def test_sim_multibfs_null_patterns_and_refusals(lib, streams, P):
    """every combination of NULL outputs writes exactly the others; the refusals come back before anything is written; k == 0"""
    pkg = load_pkg()
    n, k = 400, 70
    pp = make_pp(lib, n, P)
    pp.apply(streams.random_stream(n, 3000, seed=6))
    L, e = pp.L, pp.partition(P - 1)
    for fn, h, g in ((L.pppcsr_multi_bfs, pp.h, pp), (L.ppcsr_multi_bfs, e.h, One(e))):
        m_n = g.get_n()
        q = sources_for(g, k, 3)
        states = partition_states(g)
        m = model_multi_bfs(*global_edges(states), m_n, q)
        for mask in itertools.product((False, True), repeat=5):
            lv = np.full((k, m_n), 77, np.uint32)
            reached, far = np.full(k, 77, np.uint64), np.full(k, 77, np.uint64)
            ecc, harm = np.full(k, 77, np.uint32), np.full(k, 77.0, np.float64)
            bufs = (lv, reached, far, ecc, harm)
            rc = fn(h, q.ctypes.data, k, *[b.ctypes.data if on else None for b, on in zip(bufs, mask)], None)
            if not any(mask):
                assert rc == EINVAL and "null outputs" in L.ppcsr_last_error().decode()
                continue
            assert rc == 0, mask
            want = (m["levels"], np.array(m["reached"], np.uint64), np.array(m["far"], np.uint64), np.array(m["ecc"], np.uint32), m["harmonic"])
            for b, w, on in zip(bufs, want, mask):
                if on:
                    np.testing.assert_array_equal(b.view(np.uint64) if b.dtype == np.float64 else b, w.view(np.uint64) if w.dtype == np.float64 else w)
                else:
                    assert np.all(b == 77)
        out = np.full(k, 77, np.uint64)
        ms = ctypes.c_double(-1.0)
        assert fn(None, q.ctypes.data, k, None, out.ctypes.data, None, None, None, None) == EINVAL
        assert fn(h, None, k, None, out.ctypes.data, None, None, None, None) == EINVAL
        bad = q.copy()
        bad[k - 1] = m_n
        assert fn(h, bad.ctypes.data, k, None, out.ctypes.data, None, None, None, None) == EINVAL
        assert "out of range" in L.ppcsr_last_error().decode()
        bad[k - 1] = 0xFFFFFFFF
        assert fn(h, bad.ctypes.data, k, None, out.ctypes.data, None, None, None, None) == EINVAL
        assert fn(h, None, 0, None, None, None, None, None, None) == 0  # k == 0: nothing to read or write
        assert fn(h, q.ctypes.data, 0, None, out.ctypes.data, None, None, None, ctypes.byref(ms)) == 0
        assert np.all(out == 77)
        assert fn(h, q.ctypes.data, k, None, out.ctypes.data, None, None, None, ctypes.byref(ms)) == 0 and ms.value >= 0.0
        for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(g)):
            np.testing.assert_array_equal(i0, i1)
            np.testing.assert_array_equal(n0, n1)
    c = np.zeros(8, np.uint64)
    assert L.ppcsr_debug_multi_bfs_counters(None, c.ctypes.data) == EINVAL
    assert L.ppcsr_debug_multi_bfs_counters(e.h, None) == EINVAL
    assert L.ppcsr_debug_multi_bfs_counters(e.h, c.ctypes.data) == 0 and c[0] == 2
    with pytest.raises(pkg.PpcsrError):
        pp.multi_bfs([n])
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), lib=lib)
    q = np.array([1], np.uint32)
    out = np.full(1, 77, np.uint64)
    assert L.pppcsr_multi_bfs(loc.h, q.ctypes.data, 1, None, out.ctypes.data, None, None, None, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode() and out[0] == 77
    # (EUNSUPPORTED for partitions on several devices needs a second device: the emulator has one)
    pp.close()


@pytest.mark.parametrize("P", [1, 3])
def test_sim_multibfs_answers_in_the_sequential_regime(lib, streams, P):
    """narrow == 0 on one partition: the call answers from streaming passes alone and equals the model over the items' own
    sources; after a batch has ended the regime the rows equal bfs again"""
    n = 500
    pp = make_pp(lib, n, P)
    s, d = streams.rmat_edges_folded(n, 9, 3000, seed=23)
    adds = streams.adds(s, d)
    pp.bulk_build_device(adds.ctypes.data, len(adds))
    e = pp.partition(P - 1)
    e.set_option("search_narrow", 0)
    assert e.stats()["narrow"] == 0
    _, _, c = check(pp, sources_for(pp, 65, 4), f"sequential P={P}", bfs_rows=0)
    assert c[3] == 0 and c[4] == 0 and c[2] == c[1] and c[2] >= 2, c
    assert e.stats()["narrow"] == 0
    pp.apply(streams.random_stream(n, 600, seed=5, p_delete=0.3))  # (routes ops to every partition: the range check runs)
    assert e.stats()["narrow"] == 1
    _, _, c = check(pp, sources_for(pp, 65, 5), f"P={P} after the regime", bfs_rows=None)
    pp.close()
