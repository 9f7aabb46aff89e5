"""CPU: the device probe of the intersection routines (PCSR.debug_isect_probe) and the constructed graphs that reach the glue code
of k_tri_edges / k_tri_long / k_common_neighbours, on the fiber SIMT emulator (tests/hostsim), which compiles the engine's own
kernel and host source.  The cases, graphs and comparisons are the ones tests/test_gpu_isect.py runs on the device
(tests/isect_cases.py, tests/isect_checks.py, tests/isect_graphs.py); everything is exact."""
import numpy as np
import pytest

import isect_checks as ck
import isect_graphs as ig
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return load_pkg().load_library(SIM_SO)


@pytest.fixture(scope="module")
def eng(lib):
    return load_pkg().PCSR(64, lib=lib)


def test_generator_presence():
    """the generator's own assertions hold with the committed seeds (they run when the sets are built), and the sizes are the
    planned ones: a few hundred cases per mode, no buffer beyond 2^16 slots, n at most 2^16"""
    c, s = ck.intersect_set(), ck.search_set()
    print(c["facts"], s["facts"])
    assert 300 <= c["facts"]["lane"] <= c["facts"]["cases"] <= 900
    assert 200 <= s["facts"]["lower_bound"] <= 900 and 200 <= s["facts"]["probe"] <= 900
    assert max(len(c["items_a"]), len(c["items_b"])) <= 1 << 16 and len(s["items"]) == 1 << 16


@pytest.mark.parametrize("mode", ["lane", "wave", "block"])
def test_sim_isect_counts(eng, mode):
    assert ck.check_intersect(eng, mode) >= 300


@pytest.mark.parametrize("mode", ["lane", "wave", "block"])
def test_sim_isect_one_buffer(eng, mode):
    ck.check_one_buffer(eng, mode)


def test_sim_isect_lower_bound(eng):
    assert ck.check_lower_bound(eng) >= 200


def test_sim_isect_probe(eng):
    assert ck.check_probe(eng) >= 200


def test_sim_isect_einval(eng):
    ck.check_einval(load_pkg(), eng)


def test_sim_isect_probe_leaves_the_engine_alone(lib):
    pkg = load_pkg()
    e = pkg.PCSR(50, lib=lib)
    e.apply(np.array([[1, 2, 3], [2, 7, 1], [1, 9, 1]], np.uint32))
    before, stats = e.state(), e.stats()
    ck.check_lower_bound(e)
    ck.check_intersect(e, "wave")
    after = e.state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and stats == e.stats()
    e.close()


def test_sim_isect_uniform_claims(lib, eng):
    """every mode once more with each wv::uni / wv::bcast of the probe kernels and of the routines verified"""
    lib.ppcsr_sim_check_uniform(1)
    try:
        for mode in ("lane", "wave", "block"):
            ck.check_intersect(eng, mode)
        ck.check_lower_bound(eng)
        ck.check_probe(eng)
    finally:
        lib.ppcsr_sim_check_uniform(0)


@pytest.mark.parametrize("P", [1, 3])
def test_sim_isect_graph(lib, streams, P):
    """the constructed graph: every route and every counter of the route model met, triangles and per-route common-neighbour
    pairs equal to the model"""
    pp = ig.build(load_pkg(), lib, streams, P, emulator=True)
    print(ig.check(pp, f"P={P}"))
    pp.close()
