"""CPU: ppcsr_bulk_build and what is built on it (pppcsr_bulk_build_device, pppcsr_repartition) against the exact host model of
tests/bulk_model.py, on the fiber SIMT emulator (tests/hostsim), which compiles the engine's own kernel and host source.  The
scenarios and the driver are the ones tests/test_gpu_bulk.py runs on the device (tests/bulk_cases.py, tests/bulk_checks.py): edges[],
nodes[] and the geometry must equal the model's bit for bit, and updates applied afterwards must stay bit-exact against an oracle
started from the model.  The emulator sorts with std::stable_sort and runs the partitions one after the other: the radix sort's key
range, the concurrent per-partition builds and the three large cases are the device file's."""
import pytest

import bulk_cases as bc
import bulk_checks as ck
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim

SIM_OPTS = dict(mode=0, opt_horizon=64, epoch_ops=1024, region_slots=64, max_horizon=32, min_horizon=4, init_horizon=8, rounds_per_sync=2,
                small_batch=0, big_grid=2, big_min=512, big_window=131072)


@pytest.fixture(scope="module")
def backend():
    build_sim()
    pkg = load_pkg()
    lib = pkg.load_library(SIM_SO)

    def tune(e):
        for k, v in SIM_OPTS.items():
            e.set_option(k, v)

    def repartition(pp, new):  # (pppcsr_repartition = these three steps; the recreated engines get the emulator-sized options first)
        (d_moved, n_moved), (d_nn, n_nn) = pp.repartition_export(new)
        for k in range(pp.num_partitions()):
            tune(pp.partition(k))
        pp.bulk_build_device(d_moved, n_moved)
        pp.set_num_neighbors_device(d_nn, n_nn)

    return ck.Backend(pkg=pkg, make=lambda n, lock: pkg.PCSR(n, lock_search=lock, lib=lib),
                      make_pp=lambda n, lock, P: pkg.PPPCSR(n, lock_search=lock, numDomain=1, partitionsPerDomain=P, lib=lib),
                      tune=tune, to_device=lambda a: (a.ctypes.data, a), repartition=repartition)


@pytest.mark.parametrize("name,lock,form", bc.single_params(bc.SMALL))
def test_sim_bulk_case(backend, streams, name, lock, form):
    ck.run_case(backend, bc.BY_NAME[name], lock, streams, form)


@pytest.mark.parametrize("lock", [True, False])
def test_sim_bulk_refused_on_a_graph_with_one_edge(backend, streams, lock):
    ck.check_refused(backend, lock, streams)


@pytest.mark.parametrize("P", [4, 32])
def test_sim_pp_bulk_build_device(backend, streams, P):
    ck.check_pp_direct(backend, P, streams)


def test_sim_repartition_empty_partition_and_one_vertex_shift(backend, streams):
    ck.check_repartition_shapes(backend, streams)
