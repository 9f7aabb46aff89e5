"""GPU: ppcsr_edge_support / ppcsr_ktruss on MI355X, all partitions on one device: exactly against the model of
tests/truss_model.py (a synchronous sub-round peel on the host) on closed forms, a triangulated cylinder, a book, RMAT scale 14
under streams and a repartition on 1, 2, 4 and 8 partitions, the constructed hub graph of tests/isect_graphs.py, and a few rounds
of batch-then-check.  The graphs and checks are shared with tests/test_sim_ktruss.py (tests/truss_checks.py)."""
import ctypes

import numpy as np
import pytest

import isect_graphs
import truss_checks as tc
from helpers import load_pkg

pytestmark = pytest.mark.gpu

GRID_WAVES = 8192  # the peel's launch: at most 2048 workgroups of four waves


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()
    return p


def maker(pkg, P):
    return lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)


@pytest.mark.parametrize("P", [1, 4])
def test_ktruss_closed_forms(pkg, P):
    tc.check_k9(maker(pkg, P))
    tc.check_closed_forms(maker(pkg, P), seed=3 + P)


@pytest.mark.parametrize("P", [1, 4])
def test_ktruss_cylinder(pkg, P):
    tc.check_cylinder(maker(pkg, P))


@pytest.mark.parametrize("P", [1, 3])
def test_ktruss_book(pkg, P):
    tc.check_book(maker(pkg, P))


def test_ktruss_rmat14_across_partitions(pkg, streams):
    """RMAT scale 14 with 120 000 adds under a mixed stream (deletes, duplicate adds, destinations >= n, a planted clique) and
    add_node, on P = 1, 2, 4 and 8 and after a repartition that leaves an empty partition: every output equal word for word.
    The first frontier is wider than the grid's waves, levels are skipped, and levels take several sub-rounds"""
    n = 1 << 14
    hard = dict(tmax=21, distinct=16, gaps=2, levels=16, max_subrounds=8, below_support=n, max_support=200, first_frontier=GRID_WAVES + 1,
                backward=1, loops=1, beyond=1)
    core, mixed = tc.rmat_stream(streams, n, 14, 120_000, seed=51, folded=False)
    results = []
    for P in (1, 2, 4, 8):
        pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
        pp.apply(core)
        pp.apply(mixed)
        pp.add_node()
        pp.apply(np.array([[n, 1, 5], [2, n, 9], [1, n, 1], [0, n, 1], [1, 2, 1], [0, 1, 1], [0, 2, 1]], np.uint32))
        pp.add_node()  # (the stream's destinations >= n name both new vertices: stored before, counted now)
        if P in (1, 8):
            mt, h, _ = tc.check(pp, f"rmat14 P={P}", **hard, **({"cross": n} if P > 1 else {}))
            assert mt["vtruss"][n] >= 4  # (n with 0, 1, 2: a K4 through the new vertex)
        results.append((pp.edge_support(), pp.ktruss()))
        if P == 4:
            pp.repartition(np.array([0, 3000, 3000, 9000], np.uint64))  # (an empty partition contributes nothing)
            tc.check(pp, "rmat14 repartitioned", identities=False, **hard)
            results.append((pp.edge_support(), pp.ktruss()))
        pp.close()
    for sup, tr in results[1:]:
        tc.same(sup, results[0][0])
        tc.same(tr, results[0][1])


@pytest.mark.parametrize("P", [1, 3])
def test_ktruss_constructed_hubs(pkg, streams, P):
    """tests/isect_graphs.py's 4000-vertex graph: 16 hubs beyond 4096 + 64 slots, their edges deferred in the support phase and
    in the peel, ranges full of destinations >= n behind the counted ones"""
    pp = isect_graphs.build(pkg, None, streams, P)
    for hub in pp.isect_hubs:
        node = pp.getNode(hub)
        assert node[1] - node[0] - 1 > tc.WAVE_SLOTS + 64
    _, _, ctr = tc.check(pp, f"hubs P={P}", tmax=6, distinct=5, beyond=10000, loops=1, below_support=1000, max_subrounds=3)
    assert ctr[6] >= 1, ctr
    pp.close()


def test_ktruss_follow_batches(pkg, streams):
    """3 rounds of: apply a batch of adds, deletes, a self-loop and a destination >= n, then both calls against the model"""
    n, P = 1 << 14, 8
    pp = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P)
    s, d = streams.rmat_edges(14, 60_000, seed=61)
    pp.apply(streams.adds(s, d))
    for r in range(3):
        s2, d2 = streams.rmat_edges(14, 20_000, seed=62 + r)
        batch = np.concatenate([streams.adds(s2, d2), streams.random_stream(n, 10_000, seed=80 + r, p_delete=0.5),
                                np.array([[r, r, 1], [r, n + r, 1]], np.uint32)])
        pp.apply(batch[np.random.default_rng(r).permutation(len(batch))])
        tc.check(pp, f"round {r}", tmax=10, distinct=8, backward=1, loops=1, beyond=1, max_subrounds=4)
    pp.close()


def test_ktruss_status_codes(pkg, streams):
    """argument errors with EINVAL, ERANGE with the rest delivered, the sequential regime refused with EUNSUPPORTED, graphs
    without an upper edge, n = 0"""
    pp = tc.check_status_codes(pkg, lambda n, P: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=P), streams, 1 << 10)
    pp.close()
    e = pkg.PCSR(0)
    edges, tmax, vtruss = e.ktruss()
    assert edges.shape == (0, 3) and tmax == 0 and len(vtruss) == 0 and e.edge_support()[1] == 0
    assert not pkg.PCSR(10).debug_ktruss_counters().any()


def test_ktruss_two_devices_refused(pkg):
    """partitions on two devices: EUNSUPPORTED, with the reason"""
    L = pkg.load_library()
    if L.ppcsr_device_count() < 2:
        pytest.skip("needs a second device")
    two = pkg.PPPCSR(1 << 10, numDomain=2, partitionsPerDomain=1, devices=[0, 1])
    count = ctypes.c_uint64()
    assert L.pppcsr_ktruss(two.h, None, 0, ctypes.byref(count), None, None, None) == tc.EUNSUPPORTED
    assert "more than one device" in L.ppcsr_last_error().decode()
    assert L.pppcsr_edge_support(two.h, None, 0, ctypes.byref(count), None, None) == tc.EUNSUPPORTED


def test_ktruss_slot_search(pkg):
    tc.check_slot_search(pkg.PCSR(8))
